"""Normal estimation without a GPU: the numpy oracle (tests/point_normals_oracle.py) against np.linalg.eigh and against
closed forms, the argument checks of the two entry points (the library loads and rejects before any HIP call), and the
Python layer's ValueErrors."""
import ctypes as C

import numpy as np
import pytest

import point_normals_oracle as NO

F = np.float32
DEGENERATE = NO.DEGENERATE


# ---- clouds ------------------------------------------------------------------------------------------------------------
def sphere_cloud(n=2000):
    v = np.random.RandomState(0).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cube_cloud(n=2000):
    """uniform on the surface of [-1, 1]^3: a face and a side per point"""
    rng = np.random.RandomState(0)
    p = rng.uniform(-1, 1, size=(n, 3))
    face = rng.randint(0, 3, size=n)
    p[np.arange(n), face] = rng.choice([-1.0, 1.0], size=n)
    return p.astype(np.float32)


def plane_cloud(n=1500):
    rng = np.random.RandomState(0)
    p = rng.uniform(-1, 1, size=(n, 3))
    p[:, 2] = 0.02 * rng.normal(size=n)
    return p.astype(np.float32)


CLOUDS = {"sphere": sphere_cloud, "cube": cube_cloud, "plane": plane_cloud}
_cache = {}


def cloud_and_neighbours(name):
    """(points, neighbour table for k = 32): the k smallest keys are its first k columns"""
    if name not in _cache:
        pts = CLOUDS[name]()
        _cache[name] = (pts, NO.neighbours(pts, 32))
    return _cache[name]


# ---- the oracle's solver against eigh ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_oracle_normals_against_eigh(name, k):
    """The oracle's fp32 normal and eigh's eigenvector of the oracle's own fp64 covariance, up to sign, are within 2e-7
    rad wherever the relative gap (l1 - l0) / l2 is at least 0.01.  Rounding a unit vector to fp32 moves it by at most
    sqrt(3) * 2^-24 = 1.03e-7; a converged fp64 solver adds about 1e-16 / gap <= 1e-14: the bound is under twice the
    first term, so a miss means the sweep count or the solver is wrong."""
    pts, nb = cloud_and_neighbours(name)
    got = NO.estimate_cloud(pts, k, "none", nb=nb)
    assert got["status"] == NO.OK
    c = NO.covariance(pts, nb, k)
    M = np.empty((len(pts), 3, 3))
    for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, i, j] = M[:, j, i] = c[n]
    w, v = np.linalg.eigh(M)
    keep = (w[:, 1] - w[:, 0]) / w[:, 2] >= 0.01
    excluded = 1.0 - keep.mean()
    n = got["normals"].astype(np.float64)
    e = v[:, :, 0]
    angle = np.arctan2(np.linalg.norm(np.cross(n, e), axis=1), np.abs((n * e).sum(axis=1)))
    print("%s k=%d: excluded %.3f %%, worst angle %.3e rad" % (name, k, 100 * excluded, angle[keep].max()))
    assert excluded <= 0.01
    assert angle[keep].max() <= 2e-7
    # the variation is eigh's, to the fp32 rounding and the solver's error
    assert np.allclose(got["variation"], w[:, 0] / w.sum(axis=1), rtol=1e-6, atol=1e-12)


# ---- closed forms --------------------------------------------------------------------------------------------------------
def grid_plane():
    g = np.arange(5) * 0.5 - 1.0
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel(), y.ravel(), np.full(25, 0.25)], axis=1).astype(np.float32)


@pytest.mark.parametrize("k", [5, 9, 16])
def test_a_grid_in_a_plane_has_exact_normals(k):
    pts = grid_plane()
    for orient in ("none", "outward"):
        got = NO.estimate_cloud(pts, k, orient)
        assert got["status"] == NO.OK
        assert (got["normals"][:, :2] == 0).all() and (np.abs(got["normals"][:, 2]) == 1).all()
        assert (got["variation"] == 0).all()
    got = NO.estimate_cloud(pts, k, "viewpoint", viewpoint=(0, 0, 5))
    assert (got["normals"] == np.array([0, 0, 1], F)).all()
    got = NO.estimate_cloud(pts, k, "viewpoint", viewpoint=(0, 0, -5))
    assert (got["normals"] == np.array([0, 0, -1], F)).all()
    assert (NO.estimate_cloud(pts, k, "none")["normals"][:, 2] == 1).all()


def test_sphere_normals_point_outward():
    pts, nb = cloud_and_neighbours("sphere")
    got = NO.estimate_cloud(pts, 16, "outward", nb=nb)
    assert got["status"] == NO.OK
    dots = (got["normals"].astype(np.float64) * pts).sum(axis=1)
    assert (dots > 0).all() and dots.min() > 0.9                   # ... and nearly radial
    inward = NO.estimate_cloud(pts, 16, "viewpoint", viewpoint=(0, 0, 0), nb=nb)
    assert (inward["normals"] == -got["normals"]).all()


def test_degenerate_neighbourhoods():
    line = np.stack([np.arange(8) * 0.25, np.arange(8) * 0.5, np.arange(8) * -0.125], axis=1).astype(np.float32)
    same = np.full((4, 3), 0.3, np.float32)
    for pts in (line, same, line[:2], line[:1]):
        for orient in ("none", "outward"):
            got = NO.estimate_cloud(pts, 8, orient)
            assert got["status"] == DEGENERATE, len(pts)
            assert (got["normals"] == 0).all() and (got["variation"] == 0).all()
    assert NO.estimate_cloud(same, 8)["neighbours"].tolist() == [[0, 1, 2, 3, -1, -1, -1, -1]] * 4    # the lower id wins
    assert NO.estimate_cloud(np.zeros((0, 3), F), 8)["status"] == NO.EMPTY
    pair = np.concatenate([same, [(1.0, 0.0, 0.0)]]).astype(np.float32)      # two distinct positions: collinear
    got = NO.estimate_cloud(pair, 8)
    assert got["status"] == DEGENERATE and (got["normals"] == 0).all()


def test_orient_none_makes_the_largest_component_positive():
    pts, nb = cloud_and_neighbours("cube")
    n = NO.estimate_cloud(pts, 8, "none", nb=nb)["normals"]
    lead = n[np.arange(len(n)), np.argmax(np.abs(n), axis=1)]
    assert (lead > 0).all()
    assert NO.flip_none(np.array([[-0.5, 0.5, 0.0], [0.5, -0.5, 0.0], [0.0, -0.6, 0.6]])).tolist() == [True, False, True]


def test_neighbours_are_the_brute_force_answer():
    rng = np.random.RandomState(3)
    pts = rng.randint(0, 4, size=(150, 3)).astype(np.float32)      # a lattice with duplicates: ties everywhere
    nb = NO.neighbours(pts, 7)
    d2 = ((pts[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(axis=2)      # exact for small integers
    for i in range(len(pts)):
        assert nb[i].tolist() == sorted(range(len(pts)), key=lambda j: (d2[i, j], j))[:7]
    assert (NO.neighbours(pts[:3], 7)[:, 3:] == -1).all() and (NO.neighbours(pts[:3], 7)[:, 0] == [0, 1, 2]).all()


# ---- ABI: rejected before any HIP call -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


BADARG, UNSUPPORTED, ALIGN = -1, -2, -3


def test_workspace_query(lib):
    q = lib.gv_points_normals_workspace_bytes
    for grid in (0, 1, 7, 128):
        sizes = [q(4, t, grid) for t in (0, 1, 1000, 100000, 1 << 24, 1 << 30)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], grid
        assert all(s % 16 == 0 for s in sizes)
    assert q(1, 1000, 0) <= q(2, 1000, 0)
    assert q(0, 10, 0) == BADARG and q(-1, 10, 0) == BADARG and q(1, -1, 0) == BADARG
    assert q(1, 10, -1) == BADARG and q(1, 10, 129) == BADARG
    assert q(65536, 10, 0) == UNSUPPORTED and q(65535, 10, 0) > 0


def test_bad_arguments_return_codes(lib):
    from gvcnn_tf_amd import _lib
    f = lib.gv_points_estimate_normals
    OUT, NONE, VIEW = _lib.GV_NORMALS_ORIENT_OUTWARD, _lib.GV_NORMALS_ORIENT_NONE, _lib.GV_NORMALS_ORIENT_VIEWPOINT
    assert (NONE, OUT, VIEW) == (0, 1, 2) and _lib.GV_POINTS_DEGENERATE_NORMAL == 0x100
    ws = lib.gv_points_normals_workspace_bytes(2, 100, 0)
    vp = (C.c_float * 3)(0.0, 0.0, 5.0)
    # (no call here is valid: a valid one would reach the device)
    good = dict(points=64, offsets=64, n=2, total=100, max_points=60, k=16, orient=OUT, viewpoint=None, grid=0,
                normals=64, neighbours=64, variation=64, ws=64, ws_bytes=ws, status=64)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["points"], a["offsets"], a["n"], a["total"], a["max_points"], a["k"], a["orient"], a["viewpoint"],
                 a["grid"], a["normals"], a["neighbours"], a["variation"], a["ws"], a["ws_bytes"], a["status"], None)
    for name in ("points", "offsets", "normals", "ws", "status"):                     # a NULL required pointer
        assert call(**{name: None, "ws_bytes": 0}) == BADARG, name
    for k in (-1, 0, 2, 33, 1 << 20):
        assert call(k=k, ws_bytes=0) == BADARG, k
    for orient in (-1, 3, 99):
        assert call(orient=orient, ws_bytes=0) == BADARG, orient
    assert call(orient=VIEW, viewpoint=None, ws_bytes=0) == BADARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i in range(3):
            v = (C.c_float * 3)(0.0, 0.0, 5.0)
            v[i] = bad
            assert call(orient=VIEW, viewpoint=C.addressof(v), ws_bytes=0) == BADARG
    for grid in (-1, 129, 1000):
        assert call(grid=grid, ws_bytes=0) == BADARG, grid
    for n, total, mp in ((0, 100, 60), (-2, 100, 60), (2, -1, 60), (2, 100, -1)):
        assert call(n=n, total=total, max_points=mp, ws_bytes=0) == BADARG
    assert call(ws_bytes=ws - 1) == BADARG and call(ws_bytes=0) == BADARG            # a workspace that is too small
    assert call(orient=VIEW, viewpoint=C.addressof(vp), ws_bytes=ws - 1) == BADARG   # (a good viewpoint gets this far)
    big = lib.gv_points_normals_workspace_bytes(65535, 100, 0)
    assert call(n=65536, ws_bytes=1 << 40) == UNSUPPORTED and call(n=65535, ws_bytes=big - 1) == BADARG
    assert call(max_points=(1 << 24) + 1) == UNSUPPORTED
    assert call(ws=72) == ALIGN                                                      # not 16-byte aligned
    assert call(offsets=68) == ALIGN                                                 # not 8-byte aligned
    for name in ("points", "normals", "neighbours", "variation", "status"):          # not 4-byte aligned
        assert call(**{name: 66}) == ALIGN, name
    assert call(k=2, ws=72) == BADARG                                                # BADARG comes first


# ---- the Python layer's errors, raised before any device call --------------------------------------------------------------
def test_python_validation():
    from gvcnn_tf_amd import render as R
    pts = sphere_cloud(20)
    for k in (0, 2, 33, -1, 16.0, "16", True, None):
        with pytest.raises(ValueError, match="k must be"):
            R.estimate_normals(pts, k=k)
    for orient in ("inward", "", None, 1):
        with pytest.raises(ValueError, match="orient must be"):
            R.estimate_normals(pts, orient=orient)
    with pytest.raises(ValueError, match="viewpoint"):
        R.estimate_normals(pts, orient="viewpoint")
    for orient in ("outward", "none"):
        with pytest.raises(ValueError, match="viewpoint"):
            R.estimate_normals(pts, orient=orient, viewpoint=(0, 0, 5))
    for vp in ((0, 0), (0, 0, float("nan")), (0, 0, float("inf")), "abc", (1e39, 0, 0), 5.0):
        with pytest.raises(ValueError, match="viewpoint"):
            R.estimate_normals(pts, orient="viewpoint", viewpoint=vp)
    for grid in (0, -1, 129, 2.0, True, "auto"):
        with pytest.raises(ValueError, match="grid must be"):
            R.estimate_normals(pts, grid=grid)
    # the constructor: a bad k, and clouds that already carry normals
    for k in (2, 33, -1, True, 16.5):
        with pytest.raises(ValueError, match="k must be"):
            R.PointBatch([pts], estimate_normals=k)
    with pytest.raises(ValueError, match="already carry normals"):
        R.PointBatch([(pts, pts)], estimate_normals=8)
    with pytest.raises(ValueError, match="non-finite point"):                        # the cloud's own checks come first
        R.PointBatch([np.full((4, 3), np.nan)], estimate_normals=8)
