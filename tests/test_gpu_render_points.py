"""Points in, on the device: the splatter against the numpy restatement of its contract (tests/render_points_oracle.py),
byte for byte in all five outputs and the status; invariance under batching, workspace splitting, the grid-size hint,
repetition and point order; the engine entry points and the PNG route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import records, render as R      # noqa: E402

import explain_ref as ref                          # noqa: E402
import render_points_oracle as PO                  # noqa: E402

DEV = torch.device("cuda:0")
F = np.float32
EMPTY, ZERO_RADIUS = gv._lib.GV_RENDER_EMPTY, gv._lib.GV_RENDER_ZERO_RADIUS


def host(t):
    torch.cuda.synchronize()
    if t.dtype in (torch.bfloat16, torch.float16):                     # compared bit for bit: keep the raw bits
        t = t.view(torch.int16)
    return t.cpu().numpy()


# ---- clouds --------------------------------------------------------------------------------------------------------
def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def lattice():
    """the plane x = 0, every 3/64 inside the unit disc, plus four anchors on the unit circle (c = 0, r = 1): seen from +x
    at 64 x 64 with fit = 1 (k = 32) the points alternate between pixel centres and pixel corners."""
    g = np.arange(-21, 22) * (3.0 / 64.0)
    y, z = np.meshgrid(g, g)
    keep = y * y + z * z <= 0.97
    pts = np.stack([np.zeros(keep.sum()), y[keep], z[keep]], axis=1)
    return np.concatenate([[(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], pts]).astype(np.float32)


SPHERE, CROWD = 5, 4                                 # positions in clouds() of the two clouds with a radius of their own


def clouds():
    """[(points, normals)]: every cloud the contract has a clause for.  Some normals are zero (they take the depth
    factor)."""
    rng = np.random.RandomState(7)

    def normals(n):
        g = unit(rng.normal(size=(n, 3)))
        g[::7] = 0.0
        return g
    two = np.array([(0.3, -0.2, 0.1), (-0.4, 0.5, -0.6)], np.float32)
    same = np.array([(0.2, 0.2, 0.2)] * 3 + [(-0.7, -0.1, 0.4)], np.float32)
    lat = lattice()
    verts, tris = R.icosphere(2)
    surf = R.sample_surface(verts, tris, 5000, seed=2)                 # five 1 024-point binning chunks
    crowd = np.concatenate([rng.uniform(-1, 1, size=(1500, 3)) * 0.12 / np.sqrt(3.0), [(1.0, 1.0, 1.0)]])
    sph = unit(rng.normal(size=(300, 3)))                              # on the unit sphere: discs cross the image's edges
    empty = np.zeros((0, 3), np.float32)
    one = np.array([(0.5, 0.5, 0.5)], np.float32)
    out = [(two, normals(2)), (same, normals(4)), (lat, normals(len(lat))), surf,
           (crowd.astype(np.float32), normals(1501)), (sph, sph.copy()), (empty, empty.copy()), (one, normals(1))]
    assert len(out[SPHERE][0]) == 300 and len(out[CROWD][0]) == 1501
    return out


CLOUDS = clouds()
REFLECT = dict(light="camera", specular=0.4, shininess=32)
SHADINGS = {"depth": {}, "wrap": dict(REFLECT), "lambert": dict(REFLECT, diffuse="lambert"),
            "two_sided": dict(REFLECT, two_sided=True)}


def renderer(V, H, W, shading="depth", **kw):
    if shading != "depth":
        kw["point_reflection"] = SHADINGS[shading]
    return R.ViewRenderer(V, H, W, device=DEV, **kw)


def rotations(mode, n, seed=3):
    return None if mode is None else R.random_rotations(n, mode, seed=seed)


def radius_vector(r, batch, radius):
    """the per-cloud radii of a case: `radius` ("auto", or pixels) for every cloud, but 0.2 for the unit-sphere cloud
    (its discs cross the edges) and 2.0 for the crowd (beyond 32 pixels at every k here: R_MAX clamps)."""
    d = r.descriptor()
    k = d["proj_scale"]
    if radius == "auto":
        v = np.array([R.auto_point_radius(len(c[0]), d["fit"], k) for c in batch], np.float32)
    else:
        v = np.full(len(batch), F(radius / k), np.float32)
    if len(batch) == len(CLOUDS):
        v[SPHERE], v[CROWD] = F(0.2), F(2.0)
    return v


def device_outputs(r, batch, rots, radius, shading):
    kw = dict(rotations=rots, radius=radius, shading="depth" if shading == "depth" else "normal")
    f32q, pid, depth = r.render_points(batch, return_buffers=True, **kw)
    got = {"point_id": host(pid), "depth": host(depth).view(np.uint32), "f32q": host(f32q), "status": r.status.copy()}
    got["u8"] = host(r.render_points_uint8(batch, **kw))
    got["f32"] = host(r.render_points(batch, quantize=False, **kw))
    return got


def check_equal(r, batch, rots, radius, shading):
    """all five outputs and the status, byte for byte"""
    if shading == "depth":
        batch = [c[0] for c in batch]
    d = r.descriptor() if shading == "depth" else r.point_descriptor()
    want = PO.render(batch, d, np.asarray(radius, np.float32), rots, "depth" if shading == "depth" else "normal")
    got = device_outputs(r, batch, rots, radius, shading)
    assert sorted(got) == sorted(want)
    for key in ("status", "point_id", "depth", "u8", "f32q", "f32"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), "%s: %d entries differ" % (key, (got[key] != want[key]).sum())
    return want


GEOMETRIES = [(1, 64, 64, {}), (3, 40, 72, {"fov": 60.0}), (4, 72, 40, {"elevation": -20.0}), (12, 48, 48, {})]
RADII = ["auto", 1.0, 3.3, 0.002]                    # pixels: R = 256, R = 845, and one below R_MIN (R = 1)
# every geometry under every rotation; the radii and the shadings go round so that each meets each geometry
GRID = [(g, rot, RADII[(g + i) % 4], list(SHADINGS)[(2 * g + i) % 4])
        for g in range(4) for i, rot in enumerate((None, "z", "so3"))]
# every radius under both kinds of shading on the first geometry
SWEEP = [(0, "so3", rad, sh) for rad in RADII for sh in ("depth", "two_sided")]


@pytest.mark.parametrize("g,rot,radius,shading", GRID + SWEEP)
def test_device_equals_oracle(g, rot, radius, shading):
    V, H, W, kw = GEOMETRIES[g]
    r = renderer(V, H, W, shading, **kw)
    want = check_equal(r, CLOUDS, rotations(rot, len(CLOUDS)), radius_vector(r, CLOUDS, radius), shading)
    assert want["status"].tolist() == [0, 0, 0, 0, 0, 0, EMPTY, ZERO_RADIUS]
    bg = np.array([255, 255, 255], np.uint8)
    for m in (6, 7):
        assert (want["point_id"][m] == -1).all() and (want["u8"][m] == bg).all()
    for m in (CROWD, SPHERE) if radius == 0.002 else (0, 1, 2, 3, CROWD, SPHERE):     # (R = 1 needs an exact hit)
        assert (want["point_id"][m] >= 0).any(), m
    sph = want["point_id"][SPHERE] >= 0                                # its discs cross the edges of the shorter side
    assert (sph[:, 0, :].any() and sph[:, -1, :].any()) if H <= W else (sph[:, :, 0].any() and sph[:, :, -1].any())


@pytest.mark.parametrize("shading", ["depth", "lambert"])
def test_auto_radius_as_a_string_and_fit_one(shading):
    """radius="auto" and one plain number through the Python layer (no per-cloud vector), on a renderer with fit = 1:
    with radius 0.2 the unit-sphere cloud's discs cross all four edges of the image."""
    r = renderer(2, 48, 48, shading, fit=1.0, fov=45.0)
    batch = CLOUDS if shading != "depth" else [c[0] for c in CLOUDS]
    d = r.descriptor() if shading == "depth" else r.point_descriptor()
    auto = np.array([R.auto_point_radius(len(c[0]), d["fit"], d["proj_scale"]) for c in CLOUDS], np.float32)
    rots = rotations("so3", len(CLOUDS), seed=9)
    want = PO.render(batch, d, auto, rots, "depth" if shading == "depth" else "normal")
    got = device_outputs(r, batch, rots, "auto", shading)
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    one = device_outputs(r, batch, rots, 0.2, shading)                         # one number for every cloud
    same = PO.render(batch, d, np.full(len(batch), 0.2, np.float32), rots, "depth" if shading == "depth" else "normal")
    sph = same["point_id"][SPHERE] >= 0                                        # the unit sphere's discs cross every edge
    assert sph[:, 0, :].any() and sph[:, -1, :].any() and sph[:, :, 0].any() and sph[:, :, -1].any()
    for key in same:
        assert one[key].tobytes() == same[key].tobytes(), key


@pytest.mark.parametrize("pixels", [1.0, 0.002, 2.5])
def test_lattice_on_centres_and_corners(pixels):
    """seen from +x at 64 x 64 with fit = 1 the lattice's points sit on pixel centres and corners: with R = 256 the four
    neighbours of a centre lie exactly on the disc's boundary, with R = 1 only a centre that is hit exactly is covered."""
    r = R.ViewRenderer(1, 64, 64, elevation=0.0, azimuths=[0.0], fit=1.0, device=DEV)
    lat = CLOUDS[2][0]
    rad = np.array([F(pixels / 32.0)], np.float32)
    want = check_equal(r, [(lat, None)], None, rad, "depth")
    covered = (want["point_id"][0, 0] >= 0).sum()
    d = r.descriptor()
    X, Y, _ = PO.project(lat, d["cameras"][0], d)
    on_centre = ((X % 256 == 128) & (Y % 256 == 128)).sum()
    on_corner = ((X % 256 == 0) & (Y % 256 == 0)).sum()
    assert on_centre > 300 and on_corner > 300
    if pixels == 0.002:
        assert covered == on_centre
    else:
        assert covered > 2 * on_centre


# ---- invariance ------------------------------------------------------------------------------------------------------
INV = dict(radius="auto", shading="normal")


@pytest.fixture(scope="module")
def inv():
    r = renderer(3, 40, 72, "wrap", fov=60.0)
    rots = R.random_rotations(len(CLOUDS), "so3", seed=4)
    batch = R.PointBatch(CLOUDS, DEV)
    first = [host(t).copy() for t in r.render_points(batch, rotations=rots, return_buffers=True, **INV)]
    assert (first[1] >= 0).any()
    first.append(r.status.copy())
    return r, rots, batch, first


def test_a_cloud_alone_equals_the_cloud_in_the_batch(inv):
    r, rots, batch, first = inv
    for i, c in enumerate(CLOUDS):
        one = [host(t) for t in r.render_points([c], rotations=rots[i:i + 1], return_buffers=True, **INV)]
        for x, y in zip(first, one + [r.status]):
            assert x[i:i + 1].tobytes() == y.tobytes(), i


def test_workspace_splitting_hint_and_repetition(inv):
    r, rots, batch, first = inv
    tiny = renderer(3, 40, 72, "wrap", fov=60.0, max_workspace_bytes=1)            # one cloud per group
    again = [host(t) for t in tiny.render_points(batch, rotations=rots, return_buffers=True, **INV)]
    again.append(tiny.status.copy())
    twice = [host(t) for t in r.render_points(batch, rotations=rots, return_buffers=True, **INV)] + [r.status.copy()]
    strided = R.PointBatch(CLOUDS, DEV)
    group = strided.group
    strided.group = lambda a, b: group(a, b)[:4] + (1,)       # the grid-size hint: one workgroup per image strides all
    hinted = [host(t) for t in r.render_points(strided, rotations=rots, return_buffers=True, **INV)] + [r.status.copy()]
    for other in (again, twice, hinted):
        assert len(other) == len(first) == 4
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()


def test_point_order_does_not_matter():
    pts, nrm = CLOUDS[3]
    perm = np.random.RandomState(1).permutation(len(pts))
    r = renderer(3, 40, 72, "wrap", fov=60.0)
    rot = R.random_rotations(1, "so3", seed=6)
    kw = dict(rotations=rot, return_buffers=True, radius=F(3.3 / r.descriptor()["proj_scale"]), shading="normal")
    u8, pid, depth = [host(t).copy() for t in r.render_points_uint8([(pts, nrm)], **kw)]
    u8p, pidp, depthp = [host(t).copy() for t in r.render_points_uint8([(pts[perm], nrm[perm])], **kw)]
    assert depth.tobytes() == depthp.tobytes()
    back = np.where(pidp >= 0, perm[np.maximum(pidp, 0)], -1)
    agree = back == pid                                                # they differ only where equal depths tie
    assert agree.mean() > 0.9 and (pid >= 0).sum() > 500
    assert (u8[agree] == u8p[agree]).all()


# ---- engine and PNG ----------------------------------------------------------------------------------------------------
def make_engine(N, V, size):
    eng = gv.GVCNN("resnet_v2_50", N, V, size, size, 10, 10, device=DEV, storage="bf16")
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, 10, seed=3, spread_scores=True)
    eng.plan.bind(P)
    eng.set_head(Hd)
    return eng


def test_engine_entry_points():
    N, V, S = 2, 3, 64
    eng = make_engine(N, V, S)
    batch = R.PointBatch([CLOUDS[3], CLOUDS[4]], DEV)
    rots = R.random_rotations(N, "z", seed=1)
    r = renderer(V, S, S, "lambert")
    kw = dict(radius=0.05, shading="normal")
    got = [host(t).copy() for t in eng.forward_points(batch, renderer=r, rotations=rots, **kw)]
    views = r.render_points(batch, rotations=rots, **kw)
    want = [host(t).copy() for t in eng.forward(views)]
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    plain = [host(t).copy() for t in eng.forward_points([c[0] for c in (CLOUDS[3], CLOUDS[4])])]      # the defaults
    default = R.ViewRenderer(V, S, S, device=DEV)
    assert plain[2].tobytes() == host(eng.forward(default.render_points(batch))[2]).tobytes() != want[2].tobytes()
    assert host(eng.embed_points(batch, renderer=r, rotations=rots, **kw)).tobytes() == \
        host(eng.embed(views)).tobytes()
    with pytest.raises(ValueError):
        eng.forward_points([CLOUDS[3]])
    with pytest.raises(ValueError):
        eng.forward_points(batch, renderer=R.ViewRenderer(V, S, S + 1, device=DEV))
    # explain_points: explain on the splatted views, complete to the tolerance of tests/test_gpu_explain.py
    ex = eng.explain_points(batch, renderer=r, rotations=rots, kind="exact", **kw)
    same = eng.explain(views, kind="exact")
    for name in ("logits", "target", "baseline", "view_contrib", "maps"):
        assert host(getattr(ex, name)).tobytes() == host(getattr(same, name)).tobytes(), name
    f = eng.final
    hw = f.h * f.w
    logits = host(ex.logits)
    k = np.argmax(logits, axis=1)
    Fs = host(eng.final_view_descriptors().to(torch.float32)).astype(np.float64).reshape(N, V, hw, f.c)
    bound_of = ref.explain(Fs, host(eng.scheme), host(eng.weight), host(eng.cls_kernel), host(eng.cls_bias), k, eng.pool,
                           eng.empty_fill, "exact")
    n_all = bound_of["view_contrib"][1].sum(1) + bound_of["baseline"][1]
    T_all = bound_of["view_contrib"][2].sum(1) + bound_of["baseline"][2]
    total = host(ex.baseline).astype(np.float64) + host(ex.maps).astype(np.float64).reshape(N, -1).sum(1)
    gap = np.abs(logits[np.arange(N), k].astype(np.float64) - total)
    assert (gap <= (2.02 * (n_all + 8) * 2.0 ** -24 + 2.0 ** -8) * T_all).all()                   # bf16 storage
    assert np.abs(host(ex.maps)).max() > 0


def test_render_points_png_decodes_to_the_uint8_render():
    r = renderer(3, 40, 56, "two_sided")
    batch = R.PointBatch([CLOUDS[3], CLOUDS[5], CLOUDS[6]], DEV)
    rots = R.random_rotations(3, "so3", seed=2)
    for kw in (dict(), dict(radius=0.08, shading="normal")):
        u8 = host(r.render_points_uint8(batch, rotations=rots, **kw))
        pngs = r.render_points_png(batch, rotations=rots, **kw)
        assert len(pngs) == 3 and all(len(p) == 3 for p in pngs)
        assert r.status.tolist() == [0, 0, EMPTY]
        for n in range(3):
            for v in range(3):
                assert np.array_equal(records.decode_png(pngs[n][v]), u8[n, v])
