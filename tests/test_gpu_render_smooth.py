"""Smooth shading on the device: vertex normals gathered per render and interpolated per coverage sample, against the
numpy restatement of the contract (tests/render_smooth_oracle.py), bit for bit: u8, quantised and exact fp32, the
sample-grid face_id and depth, status.  Images are 40 x 56: 3 x 4 tiles, ragged on both axes."""
import numpy as np
import pytest
import torch                                       # noqa: F401  (before the library, as in every GPU test file)

pytestmark = pytest.mark.gpu

from gvcnn_tf_amd import records, render as R      # noqa: E402

import render_oracle as O                          # noqa: E402
import render_ss_oracle as SS                      # noqa: E402
import render_smooth_oracle as SM                  # noqa: E402
import test_gpu_render as G                        # noqa: E402
import test_gpu_render_ss as GS                    # noqa: E402

DEV = G.DEV
host = G.host
H, W = 40, 56
KEYS = ("status", "face_id", "depth", "u8", "f32q", "f32")


def check_equal(r, batch, rotations=None, meshes=None):
    """the five outputs of the renderer against the oracle; meshes: what the oracle is given when batch is a MeshBatch."""
    want = SM.render(batch if meshes is None else meshes, r.descriptor(), rotations)
    got = GS.device_outputs(r, batch, rotations)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].tobytes() != want[k].tobytes():
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)              # says where
            raise AssertionError(k)
    return want


CASES = [  # (samples, renderer arguments, rotations): every option at least once
    (1, dict(), None),
    (2, dict(fov=60.0, diffuse="lambert", specular=0.4, shininess=32, light="camera"), "so3"),
    (4, dict(two_sided=True, light="camera"), None),
    (2, dict(fov=60.0, two_sided=True, specular=0.4, shininess=32), "so3"),
    (4, dict(fov=60.0, diffuse="lambert", specular=0.4, shininess=32, light=(1.0, -2.0, 0.5)), "so3"),
    (1, dict(diffuse="lambert", specular=1.0, shininess=1, light="camera", ambient=0.0), None),
    (1, dict(specular=0.7, shininess=128, light="camera"), "so3"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_equals_oracle(case):
    samples, kw, rot = CASES[case]
    batch = [R.icosphere(1), SM.open_patch(), G.cube()]
    r = R.ViewRenderer(3, H, W, device=DEV, samples=samples, shading="smooth", **kw)
    rots = None if rot is None else R.random_rotations(len(batch), rot, seed=case)
    want = check_equal(r, batch, rots)
    assert (want["status"] == 0).all()
    assert (want["face_id"] >= 0).sum() > 0.1 * want["face_id"].size
    ball = want["u8"][0][want["face_id"][0].reshape(3, H, samples, W, samples)[:, :, 0, :, 0] >= 0]
    assert len(np.unique(ball[:, 2])) > 20                                         # a gradient, not 80 facets' values


def test_normals_follow_the_vertex_swap():
    """Two triangles of opposite index order seen from both sides: both signs of the screen area are drawn."""
    az = [20.0, 160.0, 200.0, 340.0]
    mesh = SM.swap_quad()
    for samples in (1, 2):
        r = R.ViewRenderer(4, H, W, azimuths=az, elevation=10.0, device=DEV, samples=samples, shading="smooth",
                           specular=0.4)
        want = check_equal(r, [mesh])
        assert set(np.unique(want["face_id"])) == {-1, 0, 1}
    d = r.descriptor()
    c, scale, _ = O.normalise(mesh[0], d["fit"])
    w = O.world(mesh[0], c, scale, None)
    signs = set()
    for v in range(4):
        X, Y, _ = O.project(w, d["cameras"][v], d)
        for a, b, cc in mesh[1]:
            signs.add((int(np.sign((X[b] - X[a]) * (Y[cc] - Y[a]) - (Y[b] - Y[a]) * (X[cc] - X[a]))), v < 2))
    assert signs == {(1, True), (-1, True), (1, False), (-1, False)}


def test_corners_are_added_in_ascending_triangle_order():
    """48 thin triangles of very different areas round one apex: another order of the adds changes the apex normal's
    low bits (checked here, so the case has teeth), and the device must hit the contract's."""
    mesh = SM.fan()
    r = R.ViewRenderer(3, H, W, elevation=60.0, device=DEV, shading="smooth", diffuse="lambert", specular=0.4)
    d = r.descriptor()
    c, scale, _ = O.normalise(mesh[0], d["fit"])
    w = O.world(mesh[0], c, scale, None)
    up = SM.vertex_normals(w, mesh[1], d)
    assert up[0].tobytes() != SM.vertex_normals(w, mesh[1][::-1].copy(), d)[0].tobytes()
    assert up[0].tobytes() != SM.vertex_normals(w, mesh[1], d, reverse=True)[0].tobytes()
    want = check_equal(r, [mesh])
    assert (want["face_id"] >= 0).sum() > 200
    check_equal(R.ViewRenderer(3, H, W, elevation=60.0, device=DEV, shading="smooth", two_sided=True, samples=2), [mesh])


def test_fallback_to_the_flat_factor_and_dropped_triangles():
    sheet = SM.cancelling_sheet()
    kw = dict(device=DEV, samples=2)
    smooth = R.ViewRenderer(3, H, W, shading="smooth", diffuse="lambert", specular=0.4, **kw)
    flat = R.ViewRenderer(3, H, W, **kw)
    want = check_equal(smooth, [sheet])
    assert (want["face_id"] >= 0).sum() > 200
    a, b = GS.device_outputs(smooth, [sheet]), GS.device_outputs(flat, [sheet])
    for k in KEYS:                                                                 # every covered sample is the flat one
        assert a[k].tobytes() == b[k].tobytes(), k
    # one triangle with an index out of range (dropped, as in flat mode) and one vertex no triangle names
    verts, tris = SM.open_patch()
    verts = np.concatenate([verts, [[0.1, 0.2, 0.3]]]).astype(np.float32)
    batch = R.MeshBatch([(verts, tris), R.icosphere(0)], DEV)
    bad = tris.copy()
    bad[3, 1] = 99
    batch.tris[3, 1] = 99
    off, tid = batch.adjacency_host()                                              # built from what the device holds
    assert 3 not in tid[:off[len(verts)]].tolist() and off[len(verts)] == 3 * (len(tris) - 1)
    want = check_equal(smooth, batch, meshes=[(verts, bad), R.icosphere(0)])
    assert want["status"].tolist() == [0, 0] and not (want["face_id"][0] == 3).any() and (want["face_id"][0] == 4).any()
    flat.render(batch)
    assert flat.status.tolist() == smooth.status.tolist()
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))             # status codes as in flat mode
    point = (np.ones((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    check_equal(smooth, [empty, sheet, point])
    assert smooth.status.tolist() == [1, 0, 2]


def test_splitting_and_determinism():
    meshes = [R.icosphere(3), SM.open_patch(), G.soup(), R.icosphere(0), SM.fan(), G.cube()]
    rots = R.random_rotations(6, "so3", seed=3)
    kw = dict(device=DEV, samples=2, shading="smooth", two_sided=True, specular=0.4, light="camera")
    r = R.ViewRenderer(3, H, W, **kw)
    all6 = [host(t) for t in r.render(meshes, rotations=rots, return_buffers=True)]
    assert (all6[1] >= 0).sum() > 0.1 * all6[1].size
    calls = []
    tiny = R.ViewRenderer(3, H, W, max_workspace_bytes=1, **kw)                     # halved down to one mesh per group
    lib = tiny.lib

    class Counting:
        def __getattr__(self, name):
            if name == "gv_render_draw_smooth":
                calls.append(name)
            return getattr(lib, name)
    tiny.lib = Counting()
    batch = R.MeshBatch(meshes, DEV)
    split = [host(t) for t in tiny.render(batch, rotations=rots, return_buffers=True)]
    assert len(calls) == 6                                                         # five splits
    for x, y in zip(all6, split):
        assert x.tobytes() == y.tobytes()
    for i, m in enumerate(meshes):
        one = [host(t) for t in r.render([m], rotations=rots[i:i + 1], return_buffers=True)]
        for x, y in zip(all6, one):
            assert x[i:i + 1].tobytes() == y.tobytes()
    again = [host(r.render(batch, rotations=rots)) for _ in range(2)]
    assert again[0].tobytes() == again[1].tobytes() == all6[0].tobytes()
    u8 = [host(r.render_uint8(batch, rotations=rots)) for _ in range(2)]
    assert u8[0].tobytes() == u8[1].tobytes()


@pytest.mark.parametrize("samples", [1, 2])
def test_flat_and_smooth_agree_on_separate_triangles(samples):
    """No shared vertices, wrap, no specular, a world light: at most one u8 level apart (the interpolation weights do
    not add up to exactly one; the bound is checked on the oracle in test_render_smooth_cpu.py)."""
    mesh = SM.separate_triangles()
    smooth = R.ViewRenderer(3, H, W, device=DEV, samples=samples, shading="smooth")
    flat = R.ViewRenderer(3, H, W, device=DEV, samples=samples)
    check_equal(smooth, [mesh])                                                    # the bits, then the bound
    a, b = host(smooth.render_uint8([mesh])), host(flat.render_uint8([mesh]))
    assert (b != 255).sum() > 500
    assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("samples", [1, 2])
def test_flat_renders_are_untouched(samples):
    batch = G.meshes()
    rots = R.random_rotations(len(batch), "so3", seed=4)
    plain = R.ViewRenderer(3, H, W, fov=45.0, device=DEV, samples=samples)
    named = R.ViewRenderer(3, H, W, fov=45.0, device=DEV, samples=samples, shading="flat", light=R.DEFAULT_LIGHT,
                           diffuse="wrap", specular=0.0, shininess=16)
    a, b = GS.device_outputs(plain, batch, rots), GS.device_outputs(named, batch, rots)
    want = SS.render(batch, plain.descriptor(), rots)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes() == want[k].tobytes(), k
    assert (a["face_id"] >= 0).any()


def test_png_record_round_trip(tmp_path):
    N, V = 3, 4
    batch = [G.cube(), R.icosphere(1), G.tetra()]
    r = R.ViewRenderer(V, H, W, device=DEV, samples=2, shading="smooth", light="camera", specular=0.4)
    u8 = host(r.render_uint8(batch))
    assert len(np.unique(u8)) > 32
    path = str(tmp_path / "views.tfrecord")
    recs = [records.make_example([records.encode_png(u8[n, v]) for v in range(V)], n) for n in range(N)]
    records.write_tfrecords(path, recs)
    got, labels = next(iter(records.ViewBatcher(path, V, H, W, N, DEV, augment=False)))
    assert host(got).tobytes() == host(r.render(batch, quantize=True)).tobytes()
    assert labels.tolist() == [0, 1, 2]


def test_forward_meshes_with_a_smooth_renderer():
    N, V, size = 2, 3, 64
    eng = G.make_engine("resnet_v2_50", N, V, size, size, 10, 10, storage="bf16")
    batch = R.MeshBatch([G.cube(), R.icosphere(2)], DEV)
    r = R.ViewRenderer(V, size, size, device=DEV, shading="smooth", light="camera", diffuse="lambert", specular=0.3)
    got = [host(t).copy() for t in eng.forward_meshes(batch, renderer=r)]
    want = [host(t).copy() for t in eng.forward(r.render(batch))]
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    assert host(eng.embed_meshes(batch, renderer=r)).tobytes() == host(eng.embed(r.render(batch))).tobytes()
    plain = [host(t).copy() for t in eng.forward_meshes(batch)]                    # the default renderer: flat
    assert plain[2].tobytes() != want[2].tobytes()
