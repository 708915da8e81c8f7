"""Points in, on the host: properties of the numpy restatement of the splatting contract (tests/render_points_oracle.py)
that can be derived by hand, the loaders and the sampler, PointBatch, the argument checks of render_points and the
argument codes of the gv_points_* entry points.  No device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gvcnn_tf_amd import _lib, render as R

import render_oracle as O
import render_points_oracle as PO
from test_render_ss_cpu import desc                  # a valid gv_render_desc to spoil

F = np.float32


@pytest.fixture
def host_device(monkeypatch):
    """PointBatch and ViewRenderer with their tensors in host memory: nothing here launches anything."""
    monkeypatch.setattr(R, "_device", lambda device=None: torch.device("cpu"))


def side_view(H, W, **kw):
    """One orthographic view from +x (right = +y, up = +z), the unit sphere on the shorter side."""
    return R.ViewRenderer(1, H, W, elevation=0.0, azimuths=[0.0], fit=1.0, **kw)


ANCHORS = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]        # fix c = 0, r = 1: with fit = 1 world = input


# ---- coverage ------------------------------------------------------------------------------------------------------
def test_disc_is_the_inclusive_integer_disc(host_device):
    """63 x 63: the origin lands on the centre of pixel (31, 31) (X = Y = 31.5 * 256 = 8064); a radius of 5 pixels
    (R = 1280) puts the centres of (31 +- 3, 31 +- 4) and (31 +- 5, 31) exactly on the boundary, where they belong to it."""
    d = side_view(63, 63).descriptor()
    k = d["proj_scale"]
    assert k == 31.5
    radius = F(5.0 / k)
    cloud = np.array(ANCHORS + [(0.0, 0.0, 0.0)], np.float32)
    w = cloud.copy()
    X, Y, Z = O.project(w, d["cameras"][0], d)
    assert (int(X[2]), int(Y[2])) == (8064, 8064)
    assert PO.radii(w, d["cameras"][0], d, radius).tolist() == [1280, 1280, 1280]
    got = PO.render([cloud], d, np.array([radius], np.float32))
    assert got["status"].tolist() == [O.OK]
    want = {(i, j) for i in range(63) for j in range(63)
            if (256 * i + 128 - 8064) ** 2 + (256 * j + 128 - 8064) ** 2 <= 1280 ** 2}
    assert len(want) == 81 and {(34, 35), (28, 27), (36, 31), (31, 26)} <= want and (35, 35) not in want
    ys, xs = np.nonzero(got["point_id"][0, 0] == 2)
    assert set(zip(xs.tolist(), ys.tolist())) == want
    assert (got["depth"][0, 0][got["point_id"][0, 0] == 2] == int(Z[2])).all()      # one depth over the whole disc
    # a disc under 0.71 pixel whose centre sits on a pixel corner covers nothing; on a pixel centre, that pixel
    tiny = PO.render([cloud], d, np.array([F(0.5 / k)], np.float32))
    assert (tiny["point_id"][0, 0] == 2).sum() == 1 and tiny["point_id"][0, 0, 31, 31] == 2
    d64 = side_view(64, 64).descriptor()
    assert (PO.render([cloud], d64, np.array([F(0.5 / 32.0)], np.float32))["point_id"][0, 0] == 2).sum() == 0


def brute(X, Y, Z, Rr, H, W):
    pid = np.full((H, W), -1, np.int64)
    for j in range(H):
        for i in range(W):
            keys = [(Z[p], p) for p in range(len(X))
                    if (256 * i + 128 - X[p]) ** 2 + (256 * j + 128 - Y[p]) ** 2 <= Rr[p] ** 2]
            if keys:
                pid[j, i] = min(keys)[1]
    return pid


def test_nearer_wins_and_ties_go_to_the_lower_id():
    H = W = 12
    ok = np.ones(2, bool)
    for X, Y, Z in (([1400, 1700], [1500, 1500], [10, 5]),          # the second is nearer
                    ([1400, 1700], [1500, 1500], [7, 7]),           # a tie
                    ([1700, 1400], [1500, 1500], [7, 7])):          # the same tie, input order swapped
        Rr = [600, 600]
        pid, depth = PO.splat(np.array(X), np.array(Y), np.array(Z), np.array(Rr), ok, H, W)
        want = brute(X, Y, Z, Rr, H, W)
        assert (pid == want).all()
        both = np.zeros((H, W), bool)
        for j in range(H):
            for i in range(W):
                both[j, i] = all((256 * i + 128 - X[p]) ** 2 + (256 * j + 128 - Y[p]) ** 2 <= 600 ** 2 for p in (0, 1))
        assert both.sum() >= 4
        assert (pid[both] == (1 if Z[1] < Z[0] else 0)).all()
        assert (depth[both] == min(Z)).all() and (depth[pid < 0] == 0xFFFFFFFF).all()
    # a point that is not `ok` (non-finite world position) leaves no trace
    pid, _ = PO.splat(np.array([1400, 1700]), np.array([1500, 1500]), np.array([7, 7]), np.array([600, 600]),
                      np.array([False, True]), H, W)
    assert not (pid == 0).any() and (pid == 1).any()


# ---- shading -------------------------------------------------------------------------------------------------------
def test_depth_factor_is_monotone_and_a_zero_normal_takes_it(host_device):
    r = side_view(32, 32, point_reflection=dict(light="camera", specular=0.4, shininess=32, diffuse="lambert"))
    d = r.point_descriptor()
    Z = np.unique(np.concatenate([np.arange(0, 1 << 24, 4099), [0, 1, (1 << 24) - 2, (1 << 24) - 1]])).astype(np.uint32)
    f = PO.depth_factor(Z, d)
    assert f.dtype == np.float32 and (np.diff(f) <= 0).all() and f[0] == F(1.0) and f[-1] == F(d["ambient"])
    assert f[0] > f[len(f) // 2] > f[-1]
    n = np.zeros((len(Z), 3), np.float32)
    n[::2] = F(np.nan)
    want = PO.f32(d["color"])[None, :] * f[:, None]
    assert PO.normal_colours(n, Z, 0, d).tobytes() == want.tobytes()
    # through the whole oracle: zero normals under "normal" are the "depth" picture
    rng = np.random.RandomState(5)
    pts = np.concatenate([np.array(ANCHORS, np.float32), rng.uniform(-0.5, 0.5, size=(40, 3)).astype(np.float32)])
    rad = np.array([F(2.0 / d["proj_scale"])], np.float32)
    a = PO.render([(pts, np.zeros_like(pts))], d, rad, shading="normal")
    b = PO.render([pts], d, rad, shading="depth")
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    lit = PO.render([(pts, np.tile(F([1.0, 0.0, 0.0]), (len(pts), 1)))], d, rad, shading="normal")
    assert lit["point_id"].tobytes() == b["point_id"].tobytes() and lit["u8"].tobytes() != b["u8"].tobytes()


def test_auto_point_radius_at_its_clamps():
    fit, k = 0.9, 112.0
    assert R.auto_point_radius(400, fit, k) == F(2 * 0.9 / 20.0)
    assert R.auto_point_radius(1, fit, k) == F(32.0 / k) == R.auto_point_radius(0, fit, k)      # 1.8 > 32 / k
    assert R.auto_point_radius(10 ** 8, fit, k) == F(1.0 / k)                                     # 1.8e-4 < 1 / k
    lo, hi = (2 * fit * k) ** 2, (2 * fit * k / 32.0) ** 2                 # where the clamps start to bind
    assert R.auto_point_radius(math.ceil(lo) + 1, fit, k) == F(1.0 / k)
    assert R.auto_point_radius(math.floor(lo) - 1, fit, k) > F(1.0 / k)
    assert R.auto_point_radius(math.floor(hi) - 1, fit, k) == F(32.0 / k)
    assert R.auto_point_radius(math.ceil(hi) + 1, fit, k) < F(32.0 / k)
    assert isinstance(R.auto_point_radius(400, fit, k), np.float32)


# ---- a sampled mesh against its own render ---------------------------------------------------------------------------
def test_sampled_sphere_stays_inside_the_mesh_render_and_covers_it(host_device):
    """icosphere(2)'s 162 vertices plus 4000 surface samples, V = 3, 64 x 64, orthographic, radius "auto".  The samples
    lie on the surface and the vertices give cloud and mesh the same normalisation, so every disc's centre projects
    into the mesh's silhouette: the cloud's mask lies inside the mesh mask dilated by ceil(R / 256) + 1 pixels.
    Measured coverage of the mesh mask by the cloud (this oracle, seed 11, R = 256): 0.9727, 0.9684, 0.9679 per view; the
    assertion keeps a margin of 0.02 below it."""
    verts, tris = R.icosphere(2)
    pts, _ = R.sample_surface(verts, tris, 4000, seed=11)
    cloud = np.concatenate([verts, pts])
    d = R.ViewRenderer(3, 64, 64).descriptor()
    radius = R.auto_point_radius(len(cloud), d["fit"], d["proj_scale"])
    got = PO.render([cloud], d, np.array([radius], np.float32))
    mesh = O.render([(verts, tris)], d)
    Rr = int(PO.radii(np.zeros((1, 3), np.float32), d["cameras"][0], d, radius)[0])
    grow = -(-Rr // 256) + 1
    for v in range(3):
        mm, cm = mesh["face_id"][0, v] >= 0, got["point_id"][0, v] >= 0
        big = np.zeros_like(mm)
        for j, i in zip(*np.nonzero(mm)):
            big[max(j - grow, 0):j + grow + 1, max(i - grow, 0):i + grow + 1] = True
        assert cm.any() and not (cm & ~big).any()
        share = (cm & mm).sum() / mm.sum()
        print("view %d: R = %d, coverage of the mesh mask = %.4f" % (v, Rr, share))
        assert share >= COVERAGE[v] - 0.02


COVERAGE = (0.9727, 0.9684, 0.9679)                           # measured, see the docstring above


# ---- loaders, sampler, batch -----------------------------------------------------------------------------------------
def test_load_points_round_trips(tmp_path):
    rng = np.random.RandomState(0)
    a = rng.normal(size=(17, 6)).astype(np.float32)
    p3, p6, pc, pn3, pn6 = (tmp_path / n for n in ("a.xyz", "b.txt", "c.pts", "d.npy", "e.npy"))
    p3.write_text("# a scan\n\n" + "\n".join("%r %r\t%r" % tuple(float(x) for x in row[:3]) for row in a) + "\n")
    p6.write_text("\n".join(" ".join(repr(float(x)) for x in row) + "  # tail" for row in a))
    pc.write_text("\n".join(",".join(repr(float(x)) for x in row) for row in a) + "\n#end\n")
    np.save(pn3, a[:, :3].astype(np.float64))
    np.save(pn6, a)
    got = R.load_points(p3)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == a[:, :3].tobytes()
    assert R.load_points(str(pn3)).tobytes() == a[:, :3].tobytes()
    for path in (p6, pc, pn6):
        pts, nrm = R.load_points(path)
        assert pts.dtype == nrm.dtype == np.float32
        assert pts.tobytes() == a[:, :3].tobytes() and nrm.tobytes() == a[:, 3:].tobytes()


def test_load_points_errors(tmp_path):
    def file(name, text):
        p = tmp_path / name
        p.write_text(text)
        return p
    bad = [file("a.ply", "1 2 3\n"), file("empty.xyz", "# nothing\n\n"), file("four.xyz", "1 2 3 4\n"),
           file("ragged.xyz", "1 2 3\n1 2\n"), file("word.txt", "1 2 three\n"), file("nan.pts", "1 2 nan\n"),
           file("inf.pts", "1 2 1e60\n"), tmp_path / "missing.npy"]
    for i, arr in enumerate((np.zeros((4, 4)), np.zeros(3), np.zeros((0, 3)), np.full((2, 3), np.inf),
                             np.array([["a", "b", "c"]]))):
        np.save(tmp_path / ("bad%d.npy" % i), arr)
        bad.append(tmp_path / ("bad%d.npy" % i))
    for p in bad:
        with pytest.raises(ValueError):
            R.load_points(p)


def test_sample_surface_is_deterministic_and_on_the_faces():
    verts, tris = R.icosphere(1)
    verts = verts * F(3.0) + F([10.0, -4.0, 2.0])                          # size 6, off the origin
    p, n, f = R.sample_surface(verts, tris, 2000, seed=3, return_faces=True)
    p2, n2 = R.sample_surface(verts, tris, 2000, seed=3)
    assert p.dtype == n.dtype == np.float32 and p.shape == n.shape == (2000, 3)
    assert p.tobytes() == p2.tobytes() and n.tobytes() == n2.tobytes()
    assert R.sample_surface(verts, tris, 2000, seed=4)[0].tobytes() != p.tobytes()
    v = verts.astype(np.float64)
    a, b, c = v[tris[f, 0]], v[tris[f, 1]], v[tris[f, 2]]
    size = np.linalg.norm(v.max(0) - v.min(0))
    nf = np.cross(b - a, c - a)
    nf /= np.linalg.norm(nf, axis=1, keepdims=True)
    assert np.abs(((p - a) * nf).sum(1)).max() <= 1e-6 * size              # in the face's plane
    assert np.abs(n - nf).max() <= 1e-6
    for e0, e1, o in ((a, b, c), (b, c, a), (c, a, b)):                      # and inside its three edges
        inward = np.cross(nf, e1 - e0)
        inward /= np.linalg.norm(inward, axis=1, keepdims=True)
        assert (((p - e0) * inward).sum(1)).min() >= -1e-6 * size
    counts = np.bincount(f, minlength=len(tris))                           # equal faces: roughly equal shares
    assert counts.min() > 0 and counts.max() < 3 * 2000 / len(tris)
    assert R.sample_surface(verts, tris, 0, seed=1)[0].shape == (0, 3)
    for bad in (lambda: R.sample_surface(verts, np.zeros((0, 3), np.int32), 5),
                lambda: R.sample_surface(verts, [[0, 1, 99]], 5),
                lambda: R.sample_surface(verts, [[0, 0, 1]], 5),
                lambda: R.sample_surface(verts, tris, -1)):
        with pytest.raises(ValueError):
            bad()


def test_point_batch_packs_and_validates(host_device):
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = np.ones((2, 3), np.float64)
    e = np.zeros((0, 3), np.float32)
    batch = R.PointBatch([a, e, b])
    assert len(batch) == 3 and batch.normals is None and batch.group_normals(1) is None
    assert batch.point_offsets_host.tolist() == [0, 4, 4, 6] and batch.num_points.tolist() == [4, 0, 2]
    assert batch.points.dtype == torch.float32 and batch.points.shape == (6, 3)
    p, o, n, total, biggest = batch.group(1, 3)
    assert (p - batch.points.data_ptr(), o - batch.point_offsets.data_ptr(), n, total, biggest) == (48, 8, 2, 2, 2)
    assert batch.group(0, 3)[2:] == (3, 6, 4)
    with_n = R.PointBatch([(a, a[::-1]), (b, b)])
    assert with_n.normals.shape == (6, 3) and with_n.group_normals(1) - with_n.normals.data_ptr() == 48
    assert R.PointBatch([e]).points.shape == (1, 3)                        # an address to hand over
    for bad in ([], [(a, a), b], [a, (b, b)], [np.zeros((3, 2))], [np.zeros(3)], [(a, a[:2])], [(a, a, a)],
                [np.full((2, 3), np.nan)], [(a, np.full((4, 3), np.inf))], [a.reshape(2, 2, 3)]):
        with pytest.raises(ValueError):
            R.PointBatch(bad)


# ---- render_points: what is refused on the host ------------------------------------------------------------------------
def test_render_points_argument_errors(host_device, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("render_points reached the library before its arguments were checked")
    pts = np.random.RandomState(1).uniform(-1, 1, size=(20, 3)).astype(np.float32)
    plain, with_n = R.PointBatch([pts, pts]), R.PointBatch([(pts, pts), (pts, pts)])
    r = R.ViewRenderer(2, 32, 32)
    monkeypatch.setattr(r, "_render", no_launch)
    with pytest.raises(ValueError, match="samples"):
        R.ViewRenderer(2, 32, 32, samples=2).render_points(plain)
    for bad in (0.0, -0.1, float("nan"), float("inf"), 1e-60, "big", None, True, [0.1], [0.1, 0.2, 0.3], [0.1, -0.2],
                np.ones((2, 1))):
        with pytest.raises(ValueError, match="radius"):
            r.render_points(plain, radius=bad)
    with pytest.raises(ValueError, match="normals"):
        r.render_points(plain, shading="normal")
    with pytest.raises(ValueError, match="shading"):
        r.render_points(with_n, shading="flat")
    other = R.PointBatch([pts, pts])
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="lives on"):
        r.render_points_uint8(other)
    # what passes reaches the shared body with one fp32 radius per cloud
    seen = {}
    monkeypatch.setattr(r, "_render", lambda batch, *a, **k: seen.setdefault("batch", batch))
    assert r.render_points(with_n, radius=[0.1, 0.2], shading="normal") is with_n
    assert r._point_radii(plain, 0.05).tolist() == [float(F(0.05))] * 2
    assert r._point_radii(plain, np.array([0.1, 0.2])).dtype == np.float32
    auto = R.auto_point_radius(20, r.desc.fit, r.desc.proj_scale)
    assert r._point_radii(plain, "auto").tolist() == [float(auto)] * 2


def test_point_reflection_does_not_loosen_the_flat_checks(host_device):
    for kw in (dict(light="camera"), dict(diffuse="lambert"), dict(specular=0.4), dict(shininess=32)):
        with pytest.raises(ValueError, match="smooth"):
            R.ViewRenderer(2, 16, 16, point_reflection=dict(kw), **kw)
    for bad in (dict(diffuse="half"), dict(specular=2.0), dict(shininess=3), dict(light="sun"), dict(color=1),
                dict(light=(0, 0, 0)), "lambert"):
        with pytest.raises(ValueError):
            R.ViewRenderer(2, 16, 16, point_reflection=bad)
    r = R.ViewRenderer(2, 16, 16, point_reflection=dict(light="camera", diffuse="lambert", specular=0.4, shininess=32,
                                                         two_sided=True))
    flat, pd = r.descriptor(), r.point_descriptor()
    assert (flat["shading"], flat["diffuse"], flat["light_mode"], flat["specular"], flat["flags"] & 2) == \
        ("flat", "wrap", "world", 0.0, 0)
    assert (pd["diffuse"], pd["light_mode"], pd["specular"], pd["shininess"], pd["flags"] & 2) == \
        ("lambert", "camera", float(F(0.4)), 32, 2)
    assert pd["lights"].tobytes() == (-r.cameras_host[:, 2, :]).tobytes()
    assert (r.point_shade_desc.flags, r.point_shade_desc.shininess) == (_lib.GV_RENDER_LAMBERT, 32)
    same = R.ViewRenderer(2, 16, 16, shading="smooth", specular=0.25, light="camera")     # the renderer's own otherwise
    assert same.point_descriptor()["specular"] == 0.25 and same.point_descriptor()["light_mode"] == "camera"


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def test_points_abi_argument_codes():
    """Every rejection happens before any HIP call (this runs without a device)."""
    lib = _lib.load()
    P = 4096                                             # a 16-byte aligned stand-in address: never dereferenced
    WS = lib.gv_points_workspace_bytes(2, 4, 64, 48)
    assert WS > 0 and WS % 256 == 0
    assert lib.gv_points_workspace_bytes(0, 4, 64, 48) == -1 and lib.gv_points_workspace_bytes(2, 4, 0, 48) == -1
    assert lib.gv_points_workspace_bytes(2, 65, 64, 48) == -2 and lib.gv_points_workspace_bytes(2, 4, 64, 513) == -2
    good_radius = np.array([0.1, 0.2], np.float32)       # host memory: the one array prepare reads itself

    def prep(d, **kw):
        a = dict(pts=P, po=P, n=2, total=10, mp=5, radius=good_radius.ctypes.data, cams=P, rots=None, ws=P, wsb=WS,
                 pairs=P, status=P)
        a.update(kw)
        return lib.gv_points_prepare(a["pts"], a["po"], a["n"], a["total"], a["mp"], a["radius"],
                                     C.byref(d) if d is not None else None, a["cams"], a["rots"], a["ws"], a["wsb"],
                                     a["pairs"], a["status"], None)

    sh = _lib.RenderShading()
    sh.flags, sh.shininess, sh.specular = 0, 16, 0.5

    def draw(d, **kw):
        a = dict(pts=P, po=P, n=2, total=10, mp=5, cams=P, rots=None, ws=P, wsb=WS, bins=P, binsb=256, pairs=10,
                 output=_lib.GV_RENDER_OUT_U8, out=P, pid=None, depth=None, normals=None, shading=None, lights=None,
                 halfs=None)
        a.update(kw)
        return lib.gv_points_draw(a["pts"], a["po"], a["n"], a["total"], a["mp"], C.byref(d) if d is not None else None,
                                  a["cams"], a["rots"], a["ws"], a["wsb"], a["bins"], a["binsb"], a["pairs"],
                                  a["output"], a["out"], a["pid"], a["depth"], a["normals"],
                                  None if a["shading"] is None else C.byref(a["shading"]), a["lights"], a["halfs"], None)

    for fn in (prep, draw):
        assert fn(None) == -1
        for name in ("pts", "po", "cams", "ws"):
            assert fn(desc(), **{name: None}) == -1, name
        assert fn(desc(), n=0) == -1 and fn(desc(), total=-1) == -1 and fn(desc(), mp=-1) == -1
        assert fn(desc(), wsb=WS - 1) == -1
        for bad in (dict(height=0), dict(flags=4), dict(fit=1.5), dict(ambient=-0.1), dict(proj_scale=0.0),
                    dict(flags=_lib.GV_RENDER_PERSPECTIVE, persp_dist=1.0)):
            assert fn(desc(**bad)) == -1, bad
        assert fn(desc(height=513)) == -2 and fn(desc(width=513)) == -2 and fn(desc(num_views=65)) == -2
        assert fn(desc(), mp=(1 << 24) + 1) == -2                        # more than 2^24 points in a cloud
        assert fn(desc(), n=65536, wsb=1 << 40) == -2
        assert fn(desc(), ws=P + 8) == -3
    assert prep(desc(), pairs=None) == -1 and prep(desc(), status=None) == -1 and prep(desc(), radius=None) == -1
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        for at in (0, 1):
            r = good_radius.copy()
            r[at] = bad
            assert prep(desc(), radius=r.ctypes.data) == -1, (bad, at)
    assert draw(desc(), bins=None) == -1 and draw(desc(), out=None) == -1 and draw(desc(), output=3) == -1
    assert draw(desc(), pairs=-1) == -1 and draw(desc(), pairs=65, binsb=256) == -1
    assert draw(desc(), bins=P + 4) == -3
    assert draw(desc(), output=_lib.GV_RENDER_OUT_F32, out=P + 2) == -3
    assert draw(desc(), pid=P + 2) == -3 and draw(desc(), depth=P + 2) == -3
    lit = dict(normals=P, shading=sh, lights=P, halfs=P)                 # "normal" shading needs all four
    for name in ("shading", "lights", "halfs"):
        assert draw(desc(), **dict(lit, **{name: None})) == -1, name
    for field, value, code in (("flags", 2, -1), ("specular", 1.5, -1), ("specular", -0.1, -1), ("shininess", 0, -1),
                               ("shininess", 3, -1), ("shininess", 256, -2)):
        s2 = _lib.RenderShading()
        s2.flags, s2.shininess, s2.specular = 0, 16, 0.5
        setattr(s2, field, value)
        assert draw(desc(), **dict(lit, shading=s2)) == code, (field, value)
    assert draw(desc(), **dict(lit, normals=P + 2)) == -3
