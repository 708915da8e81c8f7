"""Anti-aliased renders on the device: S x S samples per pixel against the numpy restatement of the contract
(tests/render_ss_oracle.py), bit for bit: u8, quantised and exact fp32, the sample-grid face_id and depth, status."""
import numpy as np
import pytest
import torch                                       # noqa: F401  (before the library, as in every GPU test file)

pytestmark = pytest.mark.gpu

from gvcnn_tf_amd import records, render as R      # noqa: E402

import render_oracle as O                          # noqa: E402
import render_ss_oracle as SS                      # noqa: E402
import test_gpu_render as G                        # noqa: E402

DEV = G.DEV
host = G.host


def device_outputs(r, batch, rotations=None):
    out, face, depth = r.render(batch, rotations=rotations, return_buffers=True)
    got = {"f32q": host(out), "face_id": host(face), "depth": host(depth).view(np.uint32),
           "u8": host(r.render_uint8(batch, rotations=rotations)),
           "f32": host(r.render(batch, rotations=rotations, quantize=False)), "status": r.status.copy()}
    return got


def check_equal(r, batch, rotations=None):
    want = SS.render(batch, r.descriptor(), rotations)
    got = device_outputs(r, batch, rotations)
    S = r.samples
    assert got["face_id"].shape == (len(batch), r.V, S * r.H, S * r.W)
    for k in ("status", "face_id", "depth", "u8", "f32q", "f32"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].tobytes() != want[k].tobytes():
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)              # says where
            raise AssertionError(k)
    return want


@pytest.mark.parametrize("samples", [2, 4])
@pytest.mark.parametrize("kw,rot", [({}, None), ({"fov": 60.0, "two_sided": True}, "so3")])
def test_equals_oracle(samples, kw, rot):
    batch = G.meshes() + [SS.thin_strip()]
    r = R.ViewRenderer(3, 37, 29, device=DEV, samples=samples, **kw)               # 3 x 2 tiles, ragged on both axes
    rots = None if rot is None else R.random_rotations(len(batch), rot, seed=samples)
    want = check_equal(r, batch, rots)
    assert (want["status"] == 0).all()
    assert (want["face_id"] >= 0).sum() > 0.05 * want["face_id"].size
    dup = want["face_id"][4]                                                       # coplanar duplicates: lower id wins
    assert not np.isin(dup, [1, 2]).any() and (dup == 0).any()


def test_shared_edge_every_sample_once():
    r = R.ViewRenderer(1, 32, 32, azimuths=[0.0], elevation=0.0, fit=1.0, device=DEV, samples=4)
    want = check_equal(r, [G.quad()])
    f = want["face_id"][0, 0]
    ys, xs = np.nonzero(f >= 0)
    box = f[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    assert box.size > 0.3 * f.size and (box >= 0).all()                            # no gap along the shared diagonal
    d = r.descriptor()
    verts, tris = G.quad()
    c, scale, _ = O.normalise(verts, d["fit"])
    X, Y, Z = O.project(O.world(verts, c, scale, None), d["cameras"][0], d)
    cover = [SS.raster(X, Y, Z, np.asarray([t], np.int64), 32, 32, 4)[0] >= 0 for t in tris]
    assert not (cover[0] & cover[1]).any()                                         # and no sample claimed twice
    assert ((cover[0] | cover[1]) == (f >= 0)).all()
    assert set(np.unique(f)) == {-1, 0, 1}


@pytest.mark.parametrize("fov", [0.0, 60.0])
def test_long_lists_and_binning_grids(fov):
    """Tile lists longer than one LDS pass (256) and several binning workgroups per image at S = 4; then the grid-stride
    loop of a one-workgroup binning grid."""
    batch = [R.icosphere(4), G.dense()]
    r = R.ViewRenderer(2, 40, 48, fov=fov, device=DEV, samples=4)
    rots = R.random_rotations(2, "so3", seed=9)
    counts = SS.tile_counts(batch, r.descriptor(), rots)
    assert min(len(t) for _, t in batch) > 1024 and counts[0].max() > 256 and counts[1].max() > 256
    want = check_equal(r, batch, rots)
    assert (want["face_id"] >= 0).sum() > 0.1 * want["face_id"].size
    strided = G.stride_all_chunks(R.MeshBatch(batch, DEV))
    out, f, d = r.render(strided, rotations=rots, return_buffers=True)
    assert host(f).tobytes() == want["face_id"].tobytes()
    assert host(d).view(np.uint32).tobytes() == want["depth"].tobytes()
    assert host(out).tobytes() == want["f32q"].tobytes()


def test_one_sample_through_the_new_entry_points():
    batch = G.meshes()
    rots = R.random_rotations(len(batch), "so3", seed=4)
    plain = R.ViewRenderer(3, 37, 29, fov=45.0, device=DEV, samples=1)
    ss = R.ViewRenderer(3, 37, 29, fov=45.0, device=DEV, samples=1)
    assert not plain._ss
    ss._ss = True                                                                  # gv_render_*_ss with samples = 1
    a, b = device_outputs(plain, batch, rots), device_outputs(ss, batch, rots)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert (a["face_id"] >= 0).any()


def test_batch_invariance_and_determinism():
    A, B, C = R.icosphere(4), G.soup(), G.dense()
    r = R.ViewRenderer(3, 37, 29, device=DEV, samples=2)
    rots = R.random_rotations(3, "so3", seed=3)
    all3 = [host(t) for t in r.render([A, B, C], rotations=rots, return_buffers=True)]
    assert all3[1].shape == (3, 3, 74, 58)
    for i, m in enumerate((A, B, C)):
        one = [host(t) for t in r.render([m], rotations=rots[i:i + 1], return_buffers=True)]
        for x, y in zip(all3, one):
            assert x[i:i + 1].tobytes() == y.tobytes()
    tiny = R.ViewRenderer(3, 37, 29, device=DEV, samples=2, max_workspace_bytes=1)     # one mesh per group
    split = [host(t) for t in tiny.render([A, B, C], rotations=rots, return_buffers=True)]
    for x, y in zip(all3, split):
        assert x.tobytes() == y.tobytes()
    batch = R.MeshBatch([A, B, C], DEV)
    again = [host(r.render(batch, rotations=rots)) for _ in range(3)]
    assert again[0].tobytes() == again[1].tobytes() == again[2].tobytes() == all3[0].tobytes()
    u8 = [host(r.render_uint8(batch, rotations=rots)) for _ in range(3)]
    assert u8[0].tobytes() == u8[1].tobytes() == u8[2].tobytes()


def test_png_record_round_trip(tmp_path):
    N, V, H, W = 3, 4, 40, 48
    batch = [G.cube(), R.icosphere(1), G.tetra()]
    r = R.ViewRenderer(V, H, W, device=DEV, samples=2)
    u8 = host(r.render_uint8(batch))
    assert len(np.unique(u8)) > 8                                                  # blended silhouette values
    path = str(tmp_path / "views.tfrecord")
    recs = [records.make_example([records.encode_png(u8[n, v]) for v in range(V)], n) for n in range(N)]
    records.write_tfrecords(path, recs)
    got, labels = next(iter(records.ViewBatcher(path, V, H, W, N, DEV, augment=False)))
    assert host(got).tobytes() == host(r.render(batch, quantize=True)).tobytes()
    assert labels.tolist() == [0, 1, 2]


def test_forward_meshes_with_a_supersampling_renderer():
    N, V, size = 2, 3, 64
    eng = G.make_engine("resnet_v2_50", N, V, size, size, 10, 10, storage="bf16")
    batch = R.MeshBatch([G.cube(), R.icosphere(2)], DEV)
    r = R.ViewRenderer(V, size, size, device=DEV, samples=2)
    got = [host(t).copy() for t in eng.forward_meshes(batch, renderer=r)]
    want = [host(t).copy() for t in eng.forward(r.render(batch))]
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    plain = [host(t).copy() for t in eng.forward_meshes(batch)]                    # the default renderer: one sample
    assert plain[2].tobytes() != want[2].tobytes()
