"""Registration without a GPU: the numpy oracle (tests/points_register_oracle.py) against independent formulations (a
brute-force argmin, the cleaning oracle's tree sum, numpy's SVD), the recovery of a planted pose, the stopping rules, the
argument checks of the entry point (the library loads and rejects before any HIP call) and the Python layer's
ValueErrors."""
import ctypes as C

import numpy as np
import pytest

import points_clean_oracle as CO
import points_register_oracle as RO

F = np.float32
D = np.float64


# ---- the oracle's pieces against independent code --------------------------------------------------------------------------
def test_nearest_key_is_the_brute_force_argmin_with_ties_to_the_lower_id():
    rng = np.random.RandomState(3)
    y = rng.randint(0, 4, size=(150, 3)).astype(F)                  # a lattice with duplicates: ties everywhere
    q = rng.randint(-2, 6, size=(90, 3)).astype(F)                  # some queries outside the target's box
    keys = RO.nearest_keys(q, y)
    d2 = ((q[:, None, :].astype(D) - y[None, :, :]) ** 2).sum(axis=2)                  # exact for small integers
    want = np.argmin(d2, axis=1)                                    # numpy's argmin: the first of equal values
    assert (keys & np.uint64(0xFFFFFFFF)).tolist() == want.tolist()
    assert ((keys >> np.uint64(32)).astype(np.uint32).view(F) == d2[np.arange(len(q)), want]).all()
    assert (np.bincount(want, minlength=150) > 1).any() and len(set(map(tuple, y.tolist()))) < 150


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1025, 5000])
def test_tree_sum_equals_the_cleaning_oracles(n):
    a = np.random.RandomState(n).normal(size=(n, 3)) * 1e3
    got = RO.tree_sum(a)
    for c in range(3):
        assert got[c].tobytes() == CO.tree_sum(a[:, c]).tobytes()
    assert RO.tree_sum(a[:, 0])[0].tobytes() == CO.tree_sum(a[:, 0]).tobytes()


def test_move_is_the_stated_formula():
    T = RO.rigid(RO.axis_angle((1, 2, 3), 10.0), (0.03, -0.02, 0.05))
    p = np.random.RandomState(0).normal(size=(50, 3)).astype(F)
    q = RO.move(T, p)
    for i in (0, 17, 49):
        x, y, z = [D(v) for v in p[i]]
        for c in range(3):
            assert q[i, c] == F(((T[c, 0] * x + T[c, 1] * y) + T[c, 2] * z) + T[c, 3])
    assert np.abs(q - (p.astype(D) @ T[:3, :3].T + T[:3, 3])).max() <= 2.0 ** -23 * np.abs(q).max()


# ---- Horn against SVD ------------------------------------------------------------------------------------------------------
def kabsch(H):
    """argmax_R trace(R H) over rotations, by SVD with the determinant fix: H = sum p y^T, y ~ R p"""
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def horn_cases():
    rng = np.random.RandomState(0)
    return [rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3) for _ in range(200)]


def test_horn_equals_kabsch_on_full_rank_matrices():
    """200 random full-rank H (normal entries, scales 1e-3 .. 1e3; about half have det < 0, where the SVD route needs its
    determinant fix and the quaternion route needs nothing).  Measured: the largest entrywise |R_horn - R_svd| over the
    cases is 1.4e-14 (rounding of 8 Jacobi sweeps and of the SVD); the bound asserted is ten times that, 1.4e-13, far
    below the 1e-9 at which something other than rounding would be wrong."""
    worst, negative = 0.0, 0
    for H in horn_cases():
        R = RO.horn(H)
        negative += np.linalg.det(H) < 0
        assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-14   # a proper rotation
        worst = max(worst, np.abs(R - kabsch(H)).max())
    print("largest |R_horn - R_svd| = %.3g over 200 cases, %d with det H < 0" % (worst, negative))
    assert 50 < negative < 150
    assert worst <= 1.4e-13 < 1e-9


def test_jacobi_diagonalises_and_the_quaternion_is_canonical():
    for H in horn_cases()[:20]:
        A = RO.horn_matrix(H)
        lam, V = RO.jacobi4(A)
        assert np.abs(V.T @ A @ V - np.diag(lam)).max() <= 1e-13 * np.abs(A).max()
        assert np.allclose(np.sort(lam), np.linalg.eigvalsh(A), rtol=0, atol=1e-13 * np.abs(A).max())
        q = RO.quaternion(H)
        assert abs(np.linalg.norm(q) - 1.0) <= 1e-15 and [v for v in q if v != 0][0] > 0
    # no rotation to find: H = 0 leaves V = I, the lower column wins the tie, the identity comes out
    assert RO.quaternion(np.zeros((3, 3))).tolist() == [1.0, 0.0, 0.0, 0.0]
    assert RO.horn(np.zeros((3, 3))).tolist() == np.eye(3).tolist()
    # rank 1 (a collinear pair): still a proper rotation
    u = np.array([1.0, 2.0, 3.0])
    R = RO.horn(np.outer(u, u))
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R @ u - u).max() <= 1e-14


# ---- recovery ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recovery():
    target = RO.box_surface(1000, (1.0, 0.6, 0.3), seed=0)
    R, t = RO.axis_angle((1, 2, 3), 10.0), np.array([0.03, -0.02, 0.05])
    source = (target.astype(D) @ R.T + t).astype(F)                 # the exact rigid copy, rounded to fp32
    return source, target, RO.rigid(R, t), RO.register_pair(source, target, iterations=40)


def test_recovery_of_a_planted_pose(recovery):
    """1 000 points on a 1.0 x 0.6 x 0.3 box, its copy turned 10 degrees about (1, 2, 3) and shifted by (0.03, -0.02,
    0.05), 40 rounds, no max_distance.  The final correspondence is the identity permutation (an integer condition) and
    rmse <= 1e-6 x the largest extent: 2 sqrt(3) 2^-24 = 2.1e-7 of relative rounding in the copy and in the moved point,
    times 5.  The oracle reaches the identity permutation and stops on an exact fixed point (tolerance 0) at round 10
    with rmse 7.8e-9."""
    source, target, planted, out = recovery
    print("used %d, rmse %.3g, status %#x" % (out["used"], out["rmse"], out["status"]))
    assert out["correspondence"].tolist() == list(range(1000))
    assert out["inliers"] == 1000
    assert out["rmse"] <= 1e-6 * 1.0
    assert out["status"] == RO.CONVERGED and out["used"] < 40
    # the transform undoes the planted one
    assert np.abs(out["transform"] @ planted - np.eye(4)).max() <= 1e-6
    assert np.abs(out["moved"] - target).max() <= 1e-6
    assert out["history"][0] > 0.03 and all(b <= a for a, b in zip(out["history"], out["history"][1:]))


def test_stopping_rules(recovery):
    source, target, _, full = recovery
    one = RO.register_pair(source, target, iterations=1)
    assert one["used"] == 1 and one["status"] == RO.OK and one["rmse"] == full["history"][0]
    # a tolerance stops earlier than the exact fixed point, with the transform that entered the round
    loose = RO.register_pair(source, target, iterations=40, tolerance=5e-3)
    assert loose["status"] == RO.CONVERGED and 2 <= loose["used"] < full["used"]
    assert abs(full["history"][loose["used"] - 2] - full["history"][loose["used"] - 1]) <= 5e-3
    # max_distance: inclusive, and fewer than three inliers keep the transform
    few = RO.register_pair(source, target, iterations=5, max_distance=1e-4)
    assert few["status"] == RO.FEW_PAIRS and few["used"] == 1 and few["inliers"] < 3
    assert few["transform"].tolist() == np.eye(4).tolist() and few["moved"].tobytes() == source.tobytes()
    y = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)], F)
    p = y + np.array([(0, 0, 0.5), (0, 0, 0.5), (0, 0, 0.5), (0, 0, 1.0)], F)
    edge = RO.register_pair(p, y, iterations=1, max_distance=0.5)   # d2 == max_d2 == 0.25 three times, 1.0 once
    assert edge["inliers"] == 3 and edge["correspondence"].tolist() == [0, 1, 2, -1] and edge["rmse"] == 0.5
    # empty clouds, and a moved point that is not finite
    empty = np.zeros((0, 3), F)
    for s, t in ((empty, y), (y, empty)):
        got = RO.register_pair(s, t)
        assert got["status"] == RO.EMPTY and got["used"] == 0 and got["transform"].tolist() == np.eye(4).tolist()
    far = RO.register_pair(p, y, init=RO.rigid(np.eye(3), (1e39, 0, 0)))
    assert far["status"] == RO.NONFINITE and far["used"] == 1 and far["correspondence"].tolist() == [-1] * 4
    assert far["transform"][0, 3] == 1e39 and np.isinf(far["moved"][:, 0]).all()


# ---- the library's argument checks: no device needed ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


BADARG, UNSUPPORTED, ALIGN = -1, -2, -3


def test_workspace_query(lib):
    q = lib.gv_points_register_workspace_bytes
    for grid in (0, 1, 7, 128):
        sizes = [q(4, t, t, grid) for t in (0, 1, 1000, 100000, 1 << 24, 1 << 30)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], grid
        assert all(s % 16 == 0 for s in sizes)
        assert q(4, 1000, 10, grid) < q(4, 1000, 100000, grid) and q(4, 10, 1000, grid) < q(4, 100000, 1000, grid)
    for bad in ((0, 10, 10, 0), (-1, 10, 10, 0), (2, -1, 10, 0), (2, 10, -1, 0), (2, 10, 10, -1), (2, 10, 10, 129)):
        assert q(*bad) == BADARG, bad
    assert q(65536, 10, 10, 0) == UNSUPPORTED


def test_register_bad_arguments(lib):
    from gvcnn_tf_amd import _lib
    assert (_lib.GV_POINTS_ICP_CONVERGED, _lib.GV_POINTS_ICP_FEW_PAIRS, _lib.GV_POINTS_ICP_NONFINITE) == (
        RO.CONVERGED, RO.FEW_PAIRS, RO.NONFINITE) == (0x800, 0x1000, 0x2000)
    f = lib.gv_points_register
    ws = lib.gv_points_register_workspace_bytes(2, 100, 80, 0)
    init = (C.c_double * 32)()
    good = dict(source=64, soff=64, target=64, toff=64, n=2, total_s=100, total_t=80, max_s=60, max_t=50, normals=64,
                init=C.addressof(init), iterations=30, max_distance=float("inf"), tolerance=0.0, grid=0, transforms=64,
                rmse=64, inliers=64, used=64, corr=64, moved=64, moved_normals=64, ws=64, ws_bytes=ws, status=64)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[k] for k in order], None)
    # (no call here is valid: a valid one would reach the device)
    for name in ("source", "soff", "target", "toff", "transforms", "moved", "ws", "status"):
        assert call(**{name: None, "ws_bytes": 0}) == BADARG, name
    assert call(normals=None, ws_bytes=0) == BADARG and call(moved_normals=None, ws_bytes=0) == BADARG   # both or neither
    for kw in (dict(n=0), dict(n=-2), dict(total_s=-1), dict(total_t=-1), dict(max_s=-1), dict(max_t=-1),
               dict(iterations=0), dict(iterations=-3), dict(max_distance=-0.5), dict(max_distance=float("nan")),
               dict(tolerance=-1e-9), dict(tolerance=float("nan")), dict(grid=-1), dict(grid=129)):
        assert call(ws_bytes=0, **kw) == BADARG, kw
    assert call(ws_bytes=0) == BADARG and call(ws_bytes=ws - 1) == BADARG
    assert call(n=65536, ws_bytes=1 << 40) == UNSUPPORTED
    assert call(max_s=(1 << 24) + 1) == UNSUPPORTED and call(max_t=(1 << 24) + 1) == UNSUPPORTED
    assert call(ws=72) == ALIGN
    for name in ("soff", "toff", "transforms", "rmse"):
        assert call(**{name: 68}) == ALIGN, name
    for name in ("source", "target", "normals", "inliers", "used", "corr", "moved", "moved_normals", "status"):
        assert call(**{name: 66}) == ALIGN, name
    assert call(iterations=0, ws=72) == BADARG                      # BADARG comes first


# ---- the Python layer's errors, raised before any device call --------------------------------------------------------------
def bare_batch(n, device="cuda:0"):
    """what register and merged check before they touch the device: a batch's length, device and normals"""
    import torch
    from gvcnn_tf_amd import render as R
    b = R.PointBatch.__new__(R.PointBatch)
    b.n, b.device, b.normals = n, torch.device(device), None
    return b


def test_python_validation(monkeypatch):
    import gvcnn_tf_amd as gv
    from gvcnn_tf_amd import _lib, render as R
    assert gv.register is R.register

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    pts = RO.box_surface(20)
    for it in (0, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="iterations must be"):
            R.register(pts, pts, iterations=it)
    for md in (-1.0, float("nan"), "1", True):
        with pytest.raises(ValueError, match="max_distance must be"):
            R.register(pts, pts, max_distance=md)
    for tol in (-1e-9, float("nan"), "0", None, True):
        with pytest.raises(ValueError, match="tolerance must be"):
            R.register(pts, pts, tolerance=tol)
    for init in (np.eye(3), np.zeros((2, 4, 4)), "a", np.full((4, 4), np.nan), [1.0, 2.0]):
        with pytest.raises(ValueError, match="init must be"):
            R.register(pts, pts, init=init)
    for grid in (0, 129, 2.0, "8", True):
        with pytest.raises(ValueError, match="grid must be"):
            R.register(pts, pts, grid=grid)
    it, md, tol, init, grid = R._check_register_args(3, 30, None, 0, np.eye(4), None)
    assert (it, tol, grid) == (30, 0.0, 0) and md == np.float32(np.inf) and init.shape == (3, 4, 4) and init.dtype == D
    assert R._check_register_args(1, 5, 0.25, 1e-6, None, 7)[1:] == (np.float32(0.25), 1e-6, None, 7)
    a = bare_batch(3)
    with pytest.raises(ValueError, match="3 source clouds but 2 target"):
        a.register(bare_batch(2))
    with pytest.raises(ValueError, match="source on cuda:0 but target on cuda:1"):
        a.register(bare_batch(3, "cuda:1"))
    with pytest.raises(ValueError, match="target must be a PointBatch"):
        a.register(pts)
    with pytest.raises(ValueError, match="iterations must be"):
        a.register(bare_batch(3), iterations=0)
    with pytest.raises(ValueError, match="batches of 3 and 2"):
        R.PointBatch.merged(a, bare_batch(2))
    with pytest.raises(ValueError, match="batches on"):
        R.PointBatch.merged(a, bare_batch(3, "cuda:1"))
    with pytest.raises(ValueError, match="one PointBatch at least"):
        R.PointBatch.merged()
    b = bare_batch(3)
    b.normals = object()
    with pytest.raises(ValueError, match="all or none"):
        R.PointBatch.merged(a, b)
