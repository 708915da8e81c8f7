"""Smooth shading, on the host: the vertex-to-corner adjacency of MeshBatch, the new arguments of ViewRenderer, the
per-view light and half-vectors, the argument codes of the new C-ABI entry points and self-checks of the numpy
restatement of the contract (tests/render_smooth_oracle.py).  No device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gvcnn_tf_amd import _lib, render as R

import render_oracle as O
import render_ss_oracle as SS
import render_smooth_oracle as SM
import test_render_ss_cpu as T                      # its device-free descriptor and C-ABI stand-ins

F = np.float32


def descriptor(V, H, W, light=None, diffuse="wrap", specular=0.0, shininess=16, shading="smooth", elevation=30.0,
               azimuths=None, **kw):
    """What ViewRenderer(..., shading=...).descriptor() returns, without a device."""
    d = T.descriptor(V, H, W, elevation=elevation, azimuths=azimuths, **kw)
    az = R.default_azimuths(V) if azimuths is None else azimuths
    world = R.DEFAULT_LIGHT if light in (None, "camera") else np.asarray(light, np.float64) / np.linalg.norm(light)
    d["light"] = [float(F(x)) for x in world]
    lights, halfs = R.shading_vectors(elevation, az, "camera" if light == "camera" else world)
    d.update(shading=shading, diffuse=diffuse, light_mode="camera" if light == "camera" else "world",
             specular=float(F(specular)), shininess=shininess, lights=lights, halfs=halfs)
    return d


@pytest.fixture
def host_device(monkeypatch):
    """MeshBatch and ViewRenderer with their tensors in host memory: nothing here launches anything."""
    monkeypatch.setattr(R, "_device", lambda device=None: torch.device("cpu"))


# ---- adjacency -----------------------------------------------------------------------------------------------------
def test_vertex_adjacency_is_ascending_and_drops_bad_triangles():
    tris = [(0, 1, 2), (2, 1, 3), (0, 9, 1), (3, 3, 0), (4, 2, -1), (1, 0, 3)]      # ids 2 and 4 have a bad index
    off, tid = R.vertex_adjacency(tris, 6)
    assert off.dtype == np.int64 and tid.dtype == np.int32
    assert off.tolist() == [0, 3, 6, 8, 12, 12, 12]
    lists = [tid[off[i]:off[i + 1]].tolist() for i in range(6)]
    assert lists == [[0, 3, 5], [0, 1, 5], [0, 1], [1, 3, 3, 5], [], []]           # 3 names vertex 3 twice; 4, 5 isolated
    for li in lists:
        assert li == sorted(li)
    off, tid = R.vertex_adjacency(np.zeros((0, 3), np.int32), 2)
    assert off.tolist() == [0, 0, 0] and len(tid) == 0
    rng = np.random.RandomState(0)                                                 # against a plain loop
    t = rng.randint(-1, 41, size=(500, 3))
    off, tid = R.vertex_adjacency(t, 40)
    want = [[] for _ in range(40)]
    for k, row in enumerate(t):
        if row.min() >= 0 and row.max() < 40:
            for i in row:
                want[i].append(k)
    assert [tid[off[i]:off[i + 1]].tolist() for i in range(40)] == want


def test_mesh_batch_adjacency_rebases_under_grouping(host_device):
    meshes = [R.icosphere(0), SM.open_patch(), (np.ones((4, 3), np.float32), np.zeros((0, 3), np.int32)),
              R.icosphere(1), SM.fan(5)]
    batch = R.MeshBatch(meshes)
    assert batch._adjacency_host is None and batch._adjacency is None               # lazily built
    off, tid = batch.adjacency_host()
    vo = batch.vert_offsets_host
    assert len(off) == vo[-1] + 1 and off[0] == 0 and off[-1] == len(tid) == 3 * batch.tri_offsets_host[-1]
    assert batch.adjacency_host()[0] is off and batch.adjacency()[0] is batch.adjacency()[0]   # cached
    dev_off, dev_tid = batch.adjacency()
    assert dev_off.numpy().tolist() == off.tolist() and dev_tid.numpy().tolist() == tid.tolist()
    before = batch.group(1, 4)
    for a, b in ((0, 5), (1, 4), (3, 5), (2, 3), (4, 5)):
        p_off, p_tid, corners = batch.group_adjacency(a, b)
        i0, c0 = (p_off - dev_off.data_ptr()) // 8, (p_tid - dev_tid.data_ptr()) // 4
        assert i0 == vo[a] and corners == off[vo[b]] - off[vo[a]] and c0 == off[vo[a]]
        part = off[i0:i0 + (vo[b] - vo[a]) + 1] - off[i0]                          # what the library re-bases to
        ids = tid[c0:c0 + corners]
        want = [R.vertex_adjacency(meshes[m][1], len(meshes[m][0])) for m in range(a, b)]
        assert ids.tolist() == np.concatenate([w[1] for w in want]).tolist()       # local triangle ids, mesh after mesh
        base, k = 0, 0
        for w_off, w_tid in want:
            assert (part[k:k + len(w_off)] - base).tolist() == w_off.tolist()
            base, k = base + len(w_tid), k + len(w_off) - 1
    assert batch.group(1, 4) == before                                             # group() itself is what it was


# ---- ViewRenderer ----------------------------------------------------------------------------------------------------
def test_wrong_combinations_raise_before_anything_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    bad = [dict(shading="phong"), dict(shading=None), dict(shading="smooth", diffuse="half"), dict(diffuse="half"),
           dict(light="camera"), dict(shading="flat", light="camera"), dict(diffuse="lambert"),
           dict(specular=0.4), dict(shininess=32), dict(shading="smooth", light="sun"),
           dict(shading="smooth", specular=-0.1), dict(shading="smooth", specular=1.5),
           dict(shading="smooth", specular=float("nan")), dict(shading="smooth", specular="0.4"),
           dict(shading="smooth", shininess=0), dict(shading="smooth", shininess=3), dict(shading="smooth", shininess=256),
           dict(shading="smooth", shininess=16.0), dict(shading="smooth", shininess=-16)]
    for kw in bad:
        with pytest.raises(ValueError):
            R.ViewRenderer(2, 16, 16, **kw)


def test_descriptor_carries_the_shading_fields(host_device):
    r = R.ViewRenderer(3, 40, 56, shading="smooth", light="camera", diffuse="lambert", specular=0.4, shininess=32,
                       two_sided=True, samples=2)
    d = r.descriptor()
    assert (d["shading"], d["diffuse"], d["light_mode"], d["shininess"], d["samples"]) == ("smooth", "lambert", "camera",
                                                                                          32, 2)
    assert d["specular"] == float(F(0.4)) and d["flags"] & 2
    assert d["lights"].dtype == np.float32 and d["lights"].shape == (3, 3) and d["halfs"].shape == (3, 3)
    assert d["lights"].tobytes() == (-r.cameras_host[:, 2, :]).tobytes()           # the negated forward rows
    assert d["light"] == [float(F(x)) for x in R.DEFAULT_LIGHT]                    # the flat table keeps a world light
    want = descriptor(3, 40, 56, light="camera", diffuse="lambert", specular=0.4, shininess=32, two_sided=True, samples=2)
    assert sorted(want) == sorted(d)
    for k in want:
        assert np.array_equal(np.asarray(want[k]), np.asarray(d[k])), k
    flat = R.ViewRenderer(3, 40, 56).descriptor()
    assert (flat["shading"], flat["diffuse"], flat["light_mode"], flat["specular"], flat["shininess"]) == \
        ("flat", "wrap", "world", 0.0, 16)
    sh = r.shade_desc
    assert (sh.flags, sh.shininess, sh.specular) == (_lib.GV_RENDER_LAMBERT, 32, float(F(0.4)))


def test_lights_and_half_vectors_equal_a_float64_recomputation():
    el, az = [30.0, -20.0, 0.0, 75.0], [30.0, 135.0, 270.0, 0.0]
    cams = R.camera_matrices(el, az)
    eyes = np.array([[math.cos(math.radians(e)) * math.cos(math.radians(a)),
                      math.cos(math.radians(e)) * math.sin(math.radians(a)), math.sin(math.radians(e))]
                     for e, a in zip(el, az)])
    lights, halfs = R.shading_vectors(el, az, "camera")
    assert lights.dtype == halfs.dtype == np.float32
    assert lights.tobytes() == eyes.astype(np.float32).tobytes() == (-cams[:, 2, :]).tobytes()
    assert halfs.tobytes() == (2 * eyes / np.linalg.norm(2 * eyes, axis=1, keepdims=True)).astype(np.float32).tobytes()
    sun = np.array([1.0, -2.0, 0.5])
    lights, halfs = R.shading_vectors(el, az, sun)
    unit = sun / np.linalg.norm(sun)
    assert lights.tobytes() == np.tile(unit, (4, 1)).astype(np.float32).tobytes()
    assert lights.flags["C_CONTIGUOUS"] and halfs.flags["C_CONTIGUOUS"]             # rows of three, as the kernels read them
    assert torch.from_numpy(lights).stride() == (3, 1) and torch.from_numpy(halfs).stride() == (3, 1)
    m = unit[None, :] + eyes
    assert halfs.tobytes() == (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32).tobytes()
    assert np.abs(np.linalg.norm(halfs.astype(np.float64), axis=1) - 1).max() < 1e-6
    _, halfs = R.shading_vectors(0.0, [0.0], [-1.0, 0.0, 0.0])                     # the light looks back at the eye
    assert halfs.tolist() == [[0.0, 0.0, 0.0]]


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def shading(**kw):
    s = _lib.RenderShading()
    s.flags, s.shininess, s.specular = 0, 16, 0.25
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_smooth_abi_argument_codes():
    """Every rejection happens before any HIP call (this runs without a device)."""
    lib = _lib.load()
    P = 4096                                             # a 16-byte aligned stand-in address: never dereferenced
    desc = T.desc
    WS = lib.gv_render_workspace_bytes(2, 4, 64, 48, 10)
    NB = lib.gv_render_normals_bytes(4, 0, 6)
    NB2 = lib.gv_render_normals_bytes(4, _lib.GV_RENDER_TWO_SIDED, 100)
    assert NB == 256 and NB2 == 4864 and lib.gv_render_normals_bytes(4, 0, 0) == 256          # 12 bytes, 256-aligned
    assert lib.gv_render_normals_bytes(0, 0, 6) == -1 and lib.gv_render_normals_bytes(4, 0, -1) == -1
    assert lib.gv_render_normals_bytes(4, 4, 6) == -1 and lib.gv_render_normals_bytes(65, 0, 6) == -2

    def normals(d, **kw):
        a = dict(verts=P, vo=P, tris=P, to=P, n=2, nv=6, nt=10, mt=5, cams=P, rots=None, ws=P, wsb=WS, coff=P, ctri=P,
                 corners=30, normals=P, nb=NB)
        a.update(kw)
        return lib.gv_render_vertex_normals(a["verts"], a["vo"], a["tris"], a["to"], a["n"], a["nv"], a["nt"], a["mt"],
                                            C.byref(d) if d is not None else None, a["cams"], a["rots"], a["ws"],
                                            a["wsb"], a["coff"], a["ctri"], a["corners"], a["normals"], a["nb"], None)

    def draw(d, sh=0, samples=2, **kw):
        a = dict(verts=P, vo=P, tris=P, to=P, n=2, nv=6, nt=10, mt=5, cams=P, rots=None, ws=P, wsb=WS, bins=P,
                 binsb=256, total=10, output=_lib.GV_RENDER_OUT_U8, out=P, face=None, depth=None, lights=P, halfs=P,
                 normals=P, nb=NB)
        a.update(kw)
        sh = shading() if sh == 0 else sh
        return lib.gv_render_draw_smooth(a["verts"], a["vo"], a["tris"], a["to"], a["n"], a["nv"], a["nt"], a["mt"],
                                         C.byref(d) if d is not None else None, a["cams"], a["rots"], a["ws"], a["wsb"],
                                         a["bins"], a["binsb"], a["total"], a["output"], a["out"], a["face"], a["depth"],
                                         samples, C.byref(sh) if sh is not None else None, a["lights"], a["halfs"],
                                         a["normals"], a["nb"], None)

    for fn in (normals, draw):                                             # the shared rejections
        assert fn(None) == -1
        for name in ("verts", "vo", "tris", "to", "cams", "ws", "normals"):
            assert fn(desc(), **{name: None}) == -1, name
        assert fn(desc(), n=0) == -1
        assert fn(desc(), wsb=WS - 1) == -1
        for bad in (dict(height=0), dict(flags=4), dict(fit=1.5), dict(ambient=-0.1), dict(proj_scale=0.0)):
            assert fn(desc(**bad)) == -1, bad
        assert fn(desc(height=513)) == -2 and fn(desc(num_views=65)) == -2
        assert fn(desc(), mt=(1 << 24) + 1) == -2
        assert fn(desc(), ws=P + 8) == -3
        assert fn(desc(), nb=NB - 1) == -1                                 # a normal table too small
        assert fn(desc(flags=_lib.GV_RENDER_TWO_SIDED), nv=100, nb=NB2 - 256) == -1          # one table per view
        assert fn(desc(), normals=P + 8) == -3
    assert normals(desc(), coff=None) == -1 and normals(desc(), ctri=None) == -1 and normals(desc(), corners=-1) == -1
    for name in ("lights", "halfs", "bins", "out"):
        assert draw(desc(), **{name: None}) == -1, name
    assert draw(desc(), sh=None) == -1
    for bad in (0, -1, 3, 5, 6, 12, 255, -(2 ** 31)):                      # shininess: a power of two ...
        assert draw(desc(), sh=shading(shininess=bad)) == -1, bad
    for big in (256, 1024, 2 ** 30):                                       # ... up to 128
        assert draw(desc(), sh=shading(shininess=big)) == -2, big
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert draw(desc(), sh=shading(specular=bad)) == -1, bad
    assert draw(desc(), sh=shading(flags=2)) == -1
    for bad in (0, 3, -4):
        assert draw(desc(), samples=bad) == -1
    assert draw(desc(), samples=8) == -2
    assert draw(desc(), output=3) == -1 and draw(desc(), total=65, binsb=256) == -1
    assert draw(desc(), bins=P + 4) == -3 and draw(desc(), face=P + 2) == -3
    assert lib.gv_abi_version() == 1


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdivisions", [0, 1])
def test_icosphere_vertex_normals_are_radial(subdivisions):
    """Every vertex of these two icospheres sits on a symmetry axis of its ring of faces, so the area-weighted sum of
    the face vectors points along the position."""
    verts, tris = R.icosphere(subdivisions)
    d = descriptor(1, 16, 16)
    c, scale, st = O.normalise(verts, d["fit"])
    w = O.world(verts, c, scale, R.random_rotations(1, "so3", seed=2)[0])
    n = SM.vertex_normals(w, tris, d)
    unit = w.astype(np.float64) / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True)
    assert n.dtype == np.float32 and np.abs(n - unit).max() < 1e-6
    d2 = descriptor(3, 16, 16, two_sided=True)                             # turned to the viewer: towards or away
    for v in range(3):
        n2 = SM.vertex_normals(w, tris, d2, v)
        fwd = d2["cameras"][v][2].astype(np.float64)
        clear = np.abs(unit @ fwd) > 0.8                                   # the whole ring faces one way
        assert clear.any() and np.abs(n2[clear] + np.sign(unit[clear] @ fwd)[:, None] * unit[clear]).max() < 1e-6


def test_oracle_normals_follow_the_adjacency_and_skip_bad_triangles():
    verts, tris = SM.open_patch()
    tris = np.concatenate([tris, [[0, 99, 1]]]).astype(np.int32)           # a bad triangle and (below) an isolated vertex
    verts = np.concatenate([verts, [[0.1, 0.2, 0.3]]]).astype(np.float32)
    d = descriptor(1, 16, 16)
    c, scale, _ = O.normalise(verts, d["fit"])
    w = O.world(verts, c, scale, None)
    n = SM.vertex_normals(w, tris, d)
    off, tid = R.vertex_adjacency(tris, len(verts))
    fv = SM.face_vectors(w, np.asarray(tris[:-1], np.int64))
    for i in range(len(verts)):                                            # the same sums, read off the CSR
        g = None
        for t in tid[off[i]:off[i + 1]]:
            g = fv[t] if g is None else g + fv[t]
        if g is None:
            assert n[i].tolist() == [0.0, 0.0, 0.0]
            continue
        nn = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        assert n[i].tobytes() == (g / np.sqrt(nn)).astype(np.float32).tobytes()
    assert off[-1] - off[-2] == 0 and n[-1].tolist() == [0.0, 0.0, 0.0]


def test_fan_apex_normal_depends_on_the_order_of_the_adds():
    verts, tris = SM.fan()
    d = descriptor(1, 16, 16)
    c, scale, _ = O.normalise(verts, d["fit"])
    w = O.world(verts, c, scale, None)
    up, down = SM.vertex_normals(w, tris, d), SM.vertex_normals(w, tris, d, reverse=True)
    assert len(tris) == 48 and up[0].tobytes() != down[0].tobytes()
    assert np.abs(up[0] - down[0]).max() < 1e-5                            # low bits only
    rev = (verts, tris[::-1].copy())                                       # the input reversed: ascending = the other way
    assert SM.vertex_normals(w, rev[1], d)[0].tobytes() == down[0].tobytes()


def test_cancelling_sheet_falls_back_to_the_flat_factor():
    mesh = SM.cancelling_sheet()
    d = descriptor(3, 40, 56, specular=0.4, diffuse="lambert")
    smooth = SM.render([mesh], d, samples=2)
    flat = SS.render([mesh], dict(d, shading="flat"), samples=2)
    assert (flat["face_id"] >= 0).sum() > 200
    for k in ("face_id", "depth", "u8", "f32q", "f32"):
        assert smooth[k].tobytes() == flat[k].tobytes(), k


@pytest.mark.parametrize("samples", [1, 2])
def test_separate_triangles_smooth_is_flat_within_one_level(samples):
    """No shared vertices, wrap, no specular, a world light: the three normals of a triangle are its own face's, so the
    interpolated normal is (b0 + b1 + b2) times it and the factor is the flat one up to rounding: the u8 renders differ
    by at most one level (the weights do not add up to exactly one)."""
    mesh = SM.separate_triangles()
    d = descriptor(3, 40, 56)
    smooth = SM.render([mesh], d, samples=samples)
    flat = SS.render([mesh], dict(d, shading="flat"), samples=samples)
    assert smooth["face_id"].tobytes() == flat["face_id"].tobytes() and (flat["face_id"] >= 0).sum() > 500
    assert np.abs(smooth["u8"].astype(np.int32) - flat["u8"].astype(np.int32)).max() <= 1
    assert np.abs(smooth["f32"] - flat["f32"]).max() < 1e-5


def test_smooth_shading_varies_inside_a_triangle_and_swaps_with_the_setup():
    d = descriptor(4, 40, 56, azimuths=[20.0, 160.0, 200.0, 340.0], elevation=10.0)
    mesh = SM.swap_quad()
    out = SM.render([mesh], d)
    verts, tris = mesh
    c, scale, _ = O.normalise(verts, d["fit"])
    w = O.world(verts, c, scale, None)
    signs = set()
    for v in range(4):
        X, Y, _ = O.project(w, d["cameras"][v], d)
        for a, b, cc in tris:
            signs.add((int(np.sign((X[b] - X[a]) * (Y[cc] - Y[a]) - (Y[b] - Y[a]) * (X[cc] - X[a]))), v < 2))
        for t in (0, 1):                                                   # a gradient across every visible triangle
            px = out["u8"][0, v][out["face_id"][0, v] == t]
            assert len(px) > 50 and len(np.unique(px[:, 2])) > 3
    assert signs == {(1, True), (-1, True), (1, False), (-1, False)}       # both signs of the area, from both sides
