"""Cleaning without a GPU: the numpy oracle (tests/points_clean_oracle.py) against independent formulations and against the
cases the contract was checked on, the passthrough clauses, the argument checks of the entry points (the library loads
and rejects before any HIP call), and the Python layer's ValueErrors."""
import ctypes as C
import math

import numpy as np
import pytest

import points_clean_oracle as CO

F = np.float32


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def planted(P, n_out, seed):
    """P points on the unit sphere, then n_out planted points at 4 to 8 radii"""
    rng = np.random.RandomState(seed)
    inliers = unit(rng.normal(size=(P, 3)))
    far = unit(rng.normal(size=(n_out, 3))) * rng.uniform(4.0, 8.0, size=(n_out, 1))
    return np.concatenate([inliers, far]).astype(F)


def lattice(n):
    g = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


# ---- the oracle against independent formulations ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1025, 5000])
def test_tree_sum_against_fsum(n):
    a = np.random.RandomState(n).uniform(0.0, 3.0, size=n)
    exact = math.fsum(a.tolist())
    assert abs(CO.tree_sum(a) - exact) <= 1e-12 * exact


def test_tree_sum_is_the_stated_tree():
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 1.0, 3.0])           # padded to 8: ((a0+a1) + (a2+a3)) + ((a4+0) + (0+0))
    assert CO.tree_sum(a) == ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + 0.0) + (0.0 + 0.0))
    assert CO.tree_sum([]) == 0.0 and CO.tree_sum([2.5]) == 2.5


def test_key_table_is_the_brute_force_answer_without_self():
    rng = np.random.RandomState(3)
    pts = rng.randint(0, 4, size=(150, 3)).astype(F)                # a lattice with duplicates: ties everywhere
    keys = CO.key_table(pts, 7)
    d2 = ((pts[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(axis=2)      # exact for small integers
    for i in range(len(pts)):
        want = sorted((j for j in range(len(pts)) if j != i), key=lambda j: (d2[i, j], j))[:7]
        assert (keys[i] & np.uint64(0xFFFFFFFF)).tolist() == want
        assert ((keys[i] >> np.uint64(32)).astype(np.uint32).view(F) == d2[i, want]).all()


def test_line_key_table_is_the_key_table_of_a_line_cloud():
    """the O(P) table the device tests use past 65 536 points, against the brute-force one; equal gaps do occur (ties)"""
    pts, perm = CO.line_cloud(300, 5)
    want = CO.key_table(pts, 1)
    assert CO.line_key_table(pts, perm).tobytes() == want.tobytes()
    x = np.sort(pts[:, 0])
    assert (pts[:, 1:] == 0).all() and len(np.unique(x)) == 300 and (np.diff(x)[1:] == np.diff(x)[:-1]).any()


def test_mean_distances_against_float64_norms():
    pts = planted(400, 0, 7)
    m = CO.mean_distances(CO.key_table(pts, 8))
    p = pts.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    d[np.arange(len(p)), np.arange(len(p))] = np.inf
    ref = np.sort(d, axis=1)[:, :8].mean(axis=1)
    assert np.allclose(m, ref, rtol=1e-6, atol=0)                   # fp32 d2 against fp64: 3 roundings of 2^-24


@pytest.mark.parametrize("voxel", [0.05, 0.25])
def test_centroids_against_a_float64_mean(voxel):
    """The integer route (frexp scale, rint, int64 sums) against a plain fp64 mean.  The contract takes a point's offset
    t = x - mn in fp32; the fixed point then adds at most 2^-30 * 2^E <= 2^-29 of the extent per member, and the three
    fp64 steps about 2^-52: against the fp64 mean of mn + t the centroid (before its one rounding to fp32) is within 2^-28
    of the extent.  Against the mean of the raw points the rounding of t itself enters, half an ulp of the extent
    (2^-24 of it at most): that bound is 2^-24 + 2^-28 of the extent, and it is measured here at about 2^-25."""
    pts = planted(3000, 0, 5)                                       # no two points tie
    got = CO.voxel_select_cloud(pts, voxel, True)
    mn = pts.min(axis=0)
    ext = float((pts.max(axis=0) - mn).max())
    t = (pts - mn[None, :]).astype(np.float64)                      # the fp32 offsets, widened
    first = np.nonzero(got["keep"])[0]
    assert len(first) > 20
    for i in first:
        members = got["keys"] == got["keys"][i]
        c64 = got["centroids64"][i]
        assert np.abs(c64 - (mn.astype(np.float64) + t[members].mean(axis=0))).max() <= 2.0 ** -28 * ext
        assert np.abs(c64 - pts[members].astype(np.float64).mean(axis=0)).max() <= (2.0 ** -24 + 2.0 ** -28) * ext
        assert got["centroids"][i].tobytes() == c64.astype(F).tobytes()


# ---- statistical outlier removal: the cases of the contract ----------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("P,n_out,seed", [(300, 3, 0), (1025, 5, 1), (2000, 10, 2)])
def test_planted_outliers_go_and_no_inlier_does(P, n_out, seed, k):
    got = CO.outlier_select_cloud(planted(P, n_out, seed), k, 2.0)
    assert got["status"] == CO.OK
    assert got["keep"][P:].sum() == 0, "a planted point was kept"
    assert (got["keep"][:P] == 1).all(), "an inlier was dropped"
    mu, sigma, T = got["stats"]
    assert 0 < mu < T and sigma > 0 and T == mu + 2.0 * sigma


def test_the_lattice_loses_its_corners():
    """7^3 lattice, k = 6: interior points have mean distance 1, faces / edges / corners more; sigma is tiny and ties
    are everywhere.  335 of 343 stay: the 8 corners go."""
    pts = lattice(7)
    got = CO.outlier_select_cloud(pts, 6, 2.0)
    assert got["keep"].sum() == 335
    corner = ((pts == 0) | (pts == 6)).all(axis=1)
    assert corner.sum() == 8 and (got["keep"][corner] == 0).all() and (got["keep"][~corner] == 1).all()


def test_coincident_points_are_all_kept():
    got = CO.outlier_select_cloud(np.full((8, 3), 0.25, F), 4, 2.0)
    assert got["keep"].tolist() == [1] * 8 and got["stats"].tolist() == [0.0, 0.0, 0.0] and got["status"] == CO.OK


def test_small_clouds():
    assert CO.outlier_select_cloud(np.zeros((0, 3), F), 4, 2.0)["status"] == CO.EMPTY
    one = CO.outlier_select_cloud(np.ones((1, 3), F), 4, 2.0)
    assert one["keep"].tolist() == [1] and one["stats"].tolist() == [0.0] * 3 and one["status"] == CO.OK
    two = CO.outlier_select_cloud(np.array([(0, 0, 0), (3, 4, 0)], F), 4, 2.0)       # k_eff = 1: both at 5
    assert two["keep"].tolist() == [1, 1] and two["stats"].tolist() == [5.0, 0.0, 5.0] and two["mean_dist"].tolist() == [5, 5]
    # std_ratio = 0 keeps what is at or below the mean
    got = CO.outlier_select_cloud(planted(300, 3, 0), 4, 0.0)
    assert 0 < got["keep"].sum() < 303 and got["stats"][2] == got["stats"][0]


# ---- voxel downsampling: properties ------------------------------------------------------------------------------------------
VOXEL_CLOUDS = {"sphere": planted(2000, 10, 2), "lattice": lattice(6),
                "flat": np.concatenate([np.random.RandomState(1).uniform(-1, 1, size=(400, 2)), np.zeros((400, 1))], axis=1).astype(F)}


@pytest.mark.parametrize("voxel", [0.05, 0.25, 0.5])
@pytest.mark.parametrize("name", sorted(VOXEL_CLOUDS))
def test_voxel_properties(name, voxel):
    pts = VOXEL_CLOUDS[name]
    got = CO.voxel_select_cloud(pts, voxel, True)
    assert got["status"] == CO.OK
    first = np.nonzero(got["keep"])[0]
    keys, h = got["keys"], np.float64(got["h"])
    assert len(set(keys[first].tolist())) == len(first) == len(set(keys.tolist()))   # one output per occupied voxel
    counts = np.array([(keys == keys[i]).sum() for i in first])
    assert counts.sum() == len(pts)
    mn = pts.min(axis=0).astype(np.float64)
    ext = pts.max(axis=0).astype(np.float64) - mn
    ulp = np.spacing(F(ext.max())).astype(np.float64)
    for i in first:
        c = np.array([(int(keys[i]) >> s) & 0x1FFFFF for s in (0, 21, 42)], np.float64)
        cen = got["centroids"][i].astype(np.float64)
        # inside the voxel's box, widened by one fp32 ulp of the extent (t / h is rounded; so is the centroid)
        assert (cen >= mn + c * h - ulp).all() and (cen <= mn + (c + 1) * h + ulp).all()
        rep = got["index"][i]
        assert keys[rep] == keys[i]                                 # the representative is a member
        assert i == np.nonzero(keys == keys[i])[0][0]               # the output sits at the lowest member id
    rest = got["keep"] == 0
    assert (got["index"][rest] == -1).all() and (got["centroids"][rest] == 0).all()


def test_a_voxel_as_large_as_the_cloud_gives_one_point():
    for name, pts in VOXEL_CLOUDS.items():
        got = CO.voxel_downsample([pts, pts[::-1]], 1.5, True)
        assert got["counts"].tolist() == [1, 1], name
        assert got["offsets"].tolist() == [0, 1, 2]
        ext = float((pts.max(axis=0) - pts.min(axis=0)).max())
        assert np.abs(got["points"][0].astype(np.float64) - pts.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -22 * ext
    absolute = CO.voxel_downsample([lattice(6)], 100.0, False)
    assert absolute["counts"].tolist() == [1] and absolute["points"].tolist() == [[2.5, 2.5, 2.5]]


def test_output_order_and_representative_on_a_lattice():
    got = CO.voxel_downsample([lattice(4)], 2.0, False)             # 2x2x2 voxels of 8 points each (the last cells hold 3)
    assert got["counts"].tolist() == [8]
    assert (np.diff(got["sels"][0]["keep"].nonzero()[0]) > 0).all()
    assert got["points"][0].tolist() == [0.5, 0.5, 0.5]             # members (0|1)^3
    assert got["index"][0] == 0                                     # all eight tie at d2 = 0.75: the lowest id wins


# ---- passthrough ---------------------------------------------------------------------------------------------------------------
def test_passthrough_clauses():
    pts = planted(50, 0, 4)
    for voxel, relative in ((0.0, False), (-1.0, False), (float("nan"), False), (float("inf"), False), (1e-30, True)):
        got = CO.voxel_select_cloud(pts, voxel, relative)
        if voxel == 1e-30:                                          # fine but valid h: the too-fine clause instead
            assert got["h"] > 0
        assert got["status"] == CO.PASSTHROUGH, voxel
        assert got["keep"].tolist() == [1] * 50 and got["index"].tolist() == list(range(50))
        assert got["centroids"].tobytes() == pts.tobytes()
    # relative to a cloud without extent: h = 0
    same = np.full((5, 3), 0.5, F)
    assert CO.voxel_select_cloud(same, 0.1, True)["status"] == CO.PASSTHROUGH
    assert CO.voxel_downsample([same], 0.1, False)["counts"].tolist() == [1]          # an absolute size: one voxel
    # the too-fine limit on two points
    two = np.array([(0.0, 0.0, 0.0), (1.0, 0.5, 0.25)], F)
    assert CO.voxel_select_cloud(two, 1e-8, True)["status"] == CO.PASSTHROUGH
    edge = CO.voxel_select_cloud(two, 2.0 ** -21, True)            # ext / h = 2^21 exactly: refused
    assert edge["status"] == CO.PASSTHROUGH
    fine = CO.voxel_select_cloud(two, 2.0 ** -20, True)            # the finest grid that fits the key
    assert fine["status"] == CO.OK and fine["keep"].tolist() == [1, 1]
    assert int(fine["keys"][1]) == (1 << 20) | ((1 << 19) << 21) | ((1 << 18) << 42)


def test_a_non_finite_cloud_passes_through():
    """only the C ABI can hand over such a cloud: the oracle's path for it"""
    bad = planted(20, 0, 1)
    bad[7, 1] = np.nan
    huge = np.array([(-3e38, 0, 0), (3e38, 0, 0)], F)               # finite points, an extent past fp32
    for pts in (bad, huge):
        for got in (CO.outlier_select_cloud(pts, 4, 2.0), CO.voxel_select_cloud(pts, 0.1, True)):
            assert got["status"] == CO.NONFINITE | CO.PASSTHROUGH
            assert (got["keep"] == 1).all()
        out = CO.voxel_downsample([pts], 0.1, True)
        assert out["points"].tobytes() == pts.tobytes() and out["index"].tolist() == list(range(len(pts)))
        out = CO.remove_outliers([pts, np.zeros((0, 3), F)], 4, 2.0)
        assert out["counts"].tolist() == [len(pts), 0] and (out["stats"] == 0).all() and (out["mean_dist"] == 0).all()


def test_compaction_carries_normals_of_the_index():
    pts = planted(500, 5, 3)
    nrm = np.random.RandomState(9).normal(size=pts.shape).astype(F)
    a = CO.remove_outliers([pts], 8, 2.0, normals=[nrm])
    assert a["normals"].tobytes() == nrm[a["index"]].tobytes() and a["points"].tobytes() == pts[a["index"]].tobytes()
    assert a["counts"][0] == 500 and (a["index"] == np.arange(500)).all()
    b = CO.voxel_downsample([pts], 0.1, True, normals=[nrm])
    assert b["normals"].tobytes() == nrm[b["index"]].tobytes() and 1 < b["counts"][0] < 505


# ---- the library's argument checks: no device needed ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


BADARG, UNSUPPORTED, ALIGN = -1, -2, -3


def test_workspace_query(lib):
    q = lib.gv_points_clean_workspace_bytes
    for grid in (0, 1, 7, 128):
        sizes = [q(4, t, grid) for t in (0, 1, 1000, 100000, 1 << 24, 1 << 30)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], grid
        assert all(s % 16 == 0 for s in sizes)
        assert all(q(4, t, grid) >= lib.gv_points_normals_workspace_bytes(4, t, grid) for t in (0, 1000, 1 << 24))
    for bad in ((0, 10, 0), (-1, 10, 0), (2, -1, 0), (2, 10, -1), (2, 10, 129)):
        assert q(*bad) == BADARG, bad
    assert q(65536, 10, 0) == UNSUPPORTED


def check_common_clauses(lib, call, pointers4, pointers8=()):
    """the clauses every cleaning call shares with the normals call (no call here is valid: a valid one would reach the
    device)"""
    ws = lib.gv_points_clean_workspace_bytes(2, 100, 0)
    for name in ("points", "offsets", "ws", "status"):
        assert call(**{name: None, "ws_bytes": 0}) == BADARG, name
    for n, total, mp in ((0, 100, 60), (-2, 100, 60), (2, -1, 60), (2, 100, -1)):
        assert call(n=n, total=total, max_points=mp, ws_bytes=0) == BADARG
    assert call(ws_bytes=0) == BADARG
    assert call(n=65536, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(max_points=(1 << 24) + 1) == UNSUPPORTED
    assert call(ws=72) == ALIGN and call(offsets=68) == ALIGN
    for name in pointers4:
        assert call(**{name: 66}) == ALIGN, name
    for name in pointers8:
        assert call(**{name: 68}) == ALIGN, name
    return ws


def test_outlier_select_bad_arguments(lib):
    from gvcnn_tf_amd import _lib
    assert (_lib.GV_POINTS_CLEAN_PASSTHROUGH, _lib.GV_POINTS_CLEAN_TABLE_FULL) == (0x200, 0x400)
    f = lib.gv_points_outlier_select
    ws = lib.gv_points_clean_workspace_bytes(2, 100, 0)
    good = dict(points=64, offsets=64, n=2, total=100, max_points=60, k=16, ratio=2.0, grid=0, keep=64, mean_dist=64,
                stats=64, ws=64, ws_bytes=ws, status=64)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["points"], a["offsets"], a["n"], a["total"], a["max_points"], a["k"], a["ratio"], a["grid"], a["keep"],
                 a["mean_dist"], a["stats"], a["ws"], a["ws_bytes"], a["status"], None)
    check_common_clauses(lib, call, ("points", "keep", "mean_dist", "status"), ("stats",))
    assert call(keep=None, ws_bytes=0) == BADARG
    for k in (-1, 0, 33, 1 << 20):
        assert call(k=k, ws_bytes=0) == BADARG, k
    for ratio in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(ratio=ratio, ws_bytes=0) == BADARG, ratio
    for grid in (-1, 129, 1000):
        assert call(grid=grid, ws_bytes=0) == BADARG, grid
    assert call(ws_bytes=ws - 1) == BADARG
    assert call(k=0, ws=72) == BADARG                                # BADARG comes first


def test_voxel_select_bad_arguments(lib):
    f = lib.gv_points_voxel_select
    ws = lib.gv_points_clean_workspace_bytes(2, 100, 0)
    voxel = (C.c_float * 2)(0.1, 0.1)
    good = dict(points=64, offsets=64, n=2, total=100, max_points=60, voxel=C.addressof(voxel), relative=1, grid=0, keep=64,
                centroids=64, index=64, ws=64, ws_bytes=ws, status=64)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["points"], a["offsets"], a["n"], a["total"], a["max_points"], a["voxel"], a["relative"], a["grid"],
                 a["keep"], a["centroids"], a["index"], a["ws"], a["ws_bytes"], a["status"], None)
    check_common_clauses(lib, call, ("points", "keep", "centroids", "index", "status"))
    for name in ("voxel", "keep", "centroids", "index"):
        assert call(**{name: None, "ws_bytes": 0}) == BADARG, name
    for relative in (-1, 2):
        assert call(relative=relative, ws_bytes=0) == BADARG
    for grid in (-1, 129):
        assert call(grid=grid, ws_bytes=0) == BADARG
    assert call(ws_bytes=ws - 1) == BADARG


def test_compact_bad_arguments(lib):
    f = lib.gv_points_compact
    good = dict(points=64, offsets=64, n=2, total=100, max_points=60, keep=64, selected=64, index=64, normals=64, status=64,
                out_points=64, out_normals=64, out_index=64, out_offsets=64, counts=64, ws=64, ws_bytes=400)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["points"], a["offsets"], a["n"], a["total"], a["max_points"], a["keep"], a["selected"], a["index"],
                 a["normals"], a["status"], a["out_points"], a["out_normals"], a["out_index"], a["out_offsets"], a["counts"],
                 a["ws"], a["ws_bytes"], None)
    check_common_clauses(lib, call, ("points", "keep", "selected", "index", "normals", "status", "out_points",
                                     "out_normals", "out_index", "counts"), ("out_offsets",))
    for name in ("keep", "out_points", "out_index", "out_offsets", "counts"):
        assert call(**{name: None, "ws_bytes": 0}) == BADARG, name
    assert call(normals=None, ws_bytes=0) == BADARG and call(out_normals=None, ws_bytes=0) == BADARG   # both or neither
    assert call(ws_bytes=399) == BADARG


# ---- the Python layer's errors, raised before any device call --------------------------------------------------------------
def test_python_validation():
    import gvcnn_tf_amd as gv
    from gvcnn_tf_amd import render as R
    assert gv.remove_outliers is R.remove_outliers and gv.voxel_downsample is R.voxel_downsample
    pts = planted(20, 0, 0)
    for k in (0, 33, -1, 16.0, "16", True, None):
        with pytest.raises(ValueError, match="k must be"):
            R.remove_outliers(pts, k=k)
    for ratio in (-1.0, float("nan"), float("inf"), "2", None, True, 1e60):
        with pytest.raises(ValueError, match="std_ratio must be"):
            R.remove_outliers(pts, std_ratio=ratio)
    for grid in (0, 129, 2.0, "8", True):
        with pytest.raises(ValueError, match="grid must be"):
            R.remove_outliers(pts, grid=grid)
    for voxel in (0.0, -0.1, float("nan"), float("inf"), "a", None, [0.1, 0.2], [[0.1]], True):
        with pytest.raises(ValueError, match="voxel"):
            R.voxel_downsample(pts, voxel)
    for relative in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="relative must be"):
            R.voxel_downsample(pts, 0.1, relative=relative)
    assert R._check_outlier_args(16, 2, None) == (16, np.float32(2.0), 0)
    v, rel = R._check_voxel_args(0.25, True, 3)
    assert v.dtype == np.float32 and v.tolist() == [0.25] * 3 and rel == 1
    assert R._check_voxel_args([0.1, 0.2], False, 2)[0].tolist() == [np.float32(0.1), np.float32(0.2)]
    with pytest.raises(ValueError, match="point_offsets"):
        R.PointBatch.from_device(None, [0, 5, 3])
    with pytest.raises(ValueError, match="points must be"):
        R.PointBatch.from_device(np.zeros((5, 3), np.float32), [0, 5])
