"""Registration on the device against the numpy restatement of its contract (tests/points_register_oracle.py), byte for
byte in transforms, rmse, inliers, rounds used, correspondence, moved points, rotated normals and status; invariance under
the grid hint, the cell order, batching, a sub-range of a batch, repetition and the order of the target's points; the chain
register -> merged -> voxel_downsample -> remove_outliers -> estimate_normals -> render against the chain of oracles; the
engine on a merged batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib, render as R         # noqa: E402

import point_normals_oracle as NO                  # noqa: E402
import points_clean_oracle as CO                   # noqa: E402
import points_register_oracle as RO                # noqa: E402
import render_points_oracle as PO                  # noqa: E402

DEV = torch.device("cuda:0")
F = np.float32
D = np.float64
EMPTY = _lib.GV_RENDER_EMPTY
CONVERGED, FEW, NONFINITE = _lib.GV_POINTS_ICP_CONVERGED, _lib.GV_POINTS_ICP_FEW_PAIRS, _lib.GV_POINTS_ICP_NONFINITE


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- the named pairs ---------------------------------------------------------------------------------------------------------
def sized(n, seed):
    return np.random.RandomState(seed).normal(size=(n, 3)).astype(F)


def posed(target, degrees, shift, seed, noise=0.0, take=None):
    """a rigid copy of `target` (optionally `take` of its points, with noise), rounded to fp32: the source of a pair"""
    rng = np.random.RandomState(seed)
    p = target if take is None else target[rng.permutation(len(target))[:take]]
    T = RO.rigid(RO.axis_angle(rng.normal(size=3), degrees), shift)
    return (p.astype(D) @ T[:3, :3].T + T[:3, 3] + noise * rng.normal(size=p.shape)).astype(F)


def named_pairs():
    """(source, target, init or None) by name: every clause of the contract that a pair can exercise"""
    pairs = {}
    for n, seed in ((255, 1), (256, 2), (257, 3), (1025, 4)):       # the tree's block edges and its second level
        target = sized(n + 40, seed)
        pairs["n%d" % n] = (posed(target, 8.0, (0.05, -0.03, 0.02), seed, 0.01, take=n), target, None)
    few = sized(40, 10)
    for t in (1, 2, 3):                                             # targets of one, two and three points
        pairs["t%d" % t] = (few, sized(t, 20 + t), None)
    pairs["empty_source"] = (np.zeros((0, 3), F), sized(30, 11), None)
    pairs["empty_target"] = (sized(30, 12), np.zeros((0, 3), F), None)
    dup = np.repeat(sized(20, 13), 3, axis=0)                       # every target point three times: the lowest id wins
    pairs["coincident"] = (posed(dup[::3], 5.0, (0.02, 0.0, 0.01), 13), dup, None)
    s = np.linspace(-1.0, 1.0, 50)
    line = np.outer(s, (1.0, 2.0, 3.0)).astype(F)
    pairs["collinear"] = ((line[::2] + F(0.01)).astype(F), line, None)         # H of rank 1
    same = sized(300, 14)
    pairs["same"] = (same, same.copy(), None)
    inside = sized(200, 15)
    for axis in range(3):                                           # a source wholly outside the target's box
        for sign in (-1.0, 1.0):
            shift = np.zeros(3)
            shift[axis] = sign * 12.0
            pairs["outside_%s%s" % ("-" if sign < 0 else "+", "xyz"[axis])] = (
                posed(inside, 3.0, shift, 16 + axis, take=60), inside, None)
    back = sized(400, 30)                                           # far off, and an init that brings it close
    moved = posed(back, 25.0, (3.0, -2.0, 1.0), 30)
    guess = np.linalg.inv(RO.rigid(RO.axis_angle(np.random.RandomState(30).normal(size=3), 20.0), (2.9, -2.0, 1.1)))
    pairs["init"] = (moved, back, guess)
    pairs["far"] = (sized(10, 31), sized(10, 32), RO.rigid(np.eye(3), (1e39, 0.0, 0.0)))     # a moved point overflows
    rng = np.random.RandomState(5)                                  # a noisy plate slid along itself: a slow pair
    g = np.stack(np.meshgrid(np.arange(30) * 0.1, np.arange(30) * 0.1, indexing="ij"), -1).reshape(-1, 2)
    plate = np.concatenate([g + rng.normal(size=g.shape) * 0.02, rng.normal(size=(900, 1)) * 0.02], axis=1).astype(F)
    pairs["slide"] = ((plate + np.array((2.5, 0.2, 0.0)) + rng.normal(size=plate.shape) * 0.01).astype(F)[::3], plate, None)
    y = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)], F)
    pairs["edge"] = (y + np.array([(0, 0, 0.5), (0, 0, 0.5), (0, 0, 0.5), (0, 0, 1.0)], F), y, None)   # d2 == 0.25 == max_d2
    return pairs


PAIRS = named_pairs()
ORDER = ["n255", "t1", "n256", "t2", "outside_-x", "coincident", "outside_+x", "empty_source", "n1025", "empty_target",
         "collinear", "outside_-y", "slide", "same", "outside_+y", "t3", "init", "outside_-z", "far", "outside_+z", "edge", "n257"]
assert sorted(ORDER) == sorted(PAIRS)
SOURCES = [PAIRS[k][0] for k in ORDER]
TARGETS = [PAIRS[k][1] for k in ORDER]
INIT = np.stack([np.eye(4) if PAIRS[k][2] is None else PAIRS[k][2] for k in ORDER]).astype(D)
NORMALS = [np.random.RandomState(50 + i).normal(size=s.shape).astype(F) for i, s in enumerate(SOURCES)]
KEYS = ("transforms", "rmse", "inliers", "used", "correspondence", "moved", "moved_normals", "status")
# (iterations, max_distance, tolerance): 0.5 is the boundary of "edge" in its first round; a max_distance of 1e-4 leaves
# fewer than 3 inliers nearly everywhere; a tolerance of 1e-6 stops most pairs early and leaves "slide" running
CASES = [(1, None, 0.0), (2, None, 0.0), (30, None, 0.0), (30, None, 1e-6), (1, 0.5, 0.0), (30, 0.5, 2e-3), (30, 1e-4, 0.0),
         (30, 3.0, 1e-6)]
_want = {}


def oracle(case, lo=0, hi=len(ORDER)):
    key = (case, lo, hi)
    if key not in _want:
        it, md, tol = case
        _want[key] = RO.register(SOURCES[lo:hi], TARGETS[lo:hi], INIT[lo:hi], it, md, tol, NORMALS[lo:hi])
    return _want[key]


def device_register_of(sources, normals, targets, init, case, grid=None):
    it, md, tol = case
    src = R.PointBatch(list(zip(sources, normals)), DEV)
    tgt = R.PointBatch(targets, DEV)
    new, transforms, (rmse, inliers, used), corr = src.register(tgt, it, md, tol, init, grid, return_info=True,
                                                                return_correspondence=True)
    total = int(src.point_offsets_host[-1])
    assert new.point_offsets_host.tolist() == src.point_offsets_host.tolist() and new.normal_status is None
    return {"transforms": host(transforms), "rmse": host(rmse), "inliers": host(inliers), "used": host(used),
            "correspondence": host(corr)[:total], "moved": host(new.points)[:total],
            "moved_normals": host(new.normals)[:total], "status": new.register_status.copy()}


def device_register(case, lo=0, hi=len(ORDER), grid=None, targets=None):
    return device_register_of(SOURCES[lo:hi], NORMALS[lo:hi], TARGETS[lo:hi] if targets is None else targets, INIT[lo:hi],
                              case, grid)


def assert_same(got, want, what=""):
    for key in KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), "%s %s: %d entries differ" % (what, key, (g != w).sum())


# ---- the device against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "it%d-md%s-tol%g" % c)
def test_register_equals_oracle(case):
    want = oracle(case)
    got = device_register(case)
    st = dict(zip(ORDER, got["status"].tolist()))
    used = dict(zip(ORDER, got["used"].tolist()))
    print(case, {k: (hex(st[k]), used[k]) for k in ORDER})
    assert_same(got, want, str(case))
    it, md, tol = case
    assert st["empty_source"] == st["empty_target"] == EMPTY and used["empty_source"] == used["empty_target"] == 0
    assert st["far"] == NONFINITE and used["far"] == 1
    if md is None:
        assert st["t1"] & FEW == 0 and st["t2"] & FEW == 0          # 40 inliers onto one point are 40 inliers
    if md == 1e-4:
        assert sum(1 for v in st.values() if v & FEW) >= 10 and st["same"] & FEW == 0
    if md == 0.5 and it == 1:
        i = ORDER.index("edge")
        assert got["inliers"][i] == 3 and got["rmse"][i] == 0.5     # d2 == max_d2 is an inlier
    if it == 30 and md is None:
        assert st["same"] == CONVERGED and used["same"] == 2 and got["rmse"][ORDER.index("same")] == 0.0
        assert st["init"] == CONVERGED and got["rmse"][ORDER.index("init")] < 1e-6
    if it == 30 and tol > 0:
        stopped = [k for k in ORDER if st[k] & CONVERGED]
        running = [k for k in ORDER if st[k] == 0 and used[k] == 30]
        assert any(2 < used[k] < 30 for k in stopped)
        if tol == 1e-6:
            assert running == ["slide"], (stopped, running)         # the tolerance stops some pairs and not others
    if it < 30:
        assert all(u <= it for u in used.values())
    # every transform is a proper rotation
    Rm = got["transforms"][:, :3, :3]
    ok = np.array([k not in ("far",) for k in ORDER])
    assert np.abs(Rm[ok] @ Rm[ok].transpose(0, 2, 1) - np.eye(3)).max() < 1e-9 and (np.linalg.det(Rm[ok]) > 0.999).all()


# Sources past 65 536 points: level 1 of the tree sums has a second block and level 2 reads more than one partial.  The
# sums run over the source alone, so targets of 64 points keep the brute-force oracle quick; a small pair goes first so
# that the large sources do not start at a multiple of 256.  LARGE_MD = 0.5 rejects some pairs and keeps most of the tree
# busy: on the oracle the two large pairs have 29 674 / 30 860, 29 707 / 30 905 and 29 711 / 30 933 inliers in rounds 1 to 3.
LARGE_MD = 0.5
_large = {}


def large_pairs():
    if not _large:
        small = sized(140, 40)
        _large["sources"] = [posed(small, 8.0, (0.05, -0.03, 0.02), 40, 0.01, take=100), sized(65536, 41), sized(65537, 42)]
        _large["targets"] = [small, sized(64, 43), sized(64, 44)]
        _large["normals"] = [np.random.RandomState(80 + i).normal(size=s.shape).astype(F)
                             for i, s in enumerate(_large["sources"])]
    return _large["sources"], _large["normals"], _large["targets"]


@pytest.mark.parametrize("md", [None, LARGE_MD])
def test_register_past_65536_source_points_equals_oracle(md):
    sources, normals, targets = large_pairs()
    case = (3, md, 0.0)
    want = RO.register(sources, targets, None, 3, md, 0.0, normals)
    assert want["used"].tolist() == [3, 3, 3] and want["status"].tolist() == [0, 0, 0]
    rounds = [RO.register(sources[1:], targets[1:], None, it, md, 0.0)["inliers"].tolist() for it in (1, 2)]
    for inliers in rounds + [want["inliers"][1:].tolist()]:         # every round: some pairs rejected, never too few
        for i in (0, 1):
            assert (3 <= inliers[i] < len(sources[1 + i])) if md else (inliers[i] == len(sources[1 + i]))
    if md:
        assert rounds == [[29674, 30860], [29707, 30905]] and want["inliers"][1:].tolist() == [29711, 30933]
    assert_same(device_register_of(sources, normals, targets, None, case), want, str(case))


# ---- nothing but speed depends on the grid or the batch ----------------------------------------------------------------
INV = (30, 3.0, 1e-6)


@pytest.fixture(scope="module")
def whole():
    return device_register(INV)


@pytest.mark.parametrize("grid", [1, 2, 7, 128])
def test_the_grid_hint_changes_nothing(whole, grid):
    """grid = 1 is brute force on the device; 128 is clamped per cloud (None is the fixture's)"""
    assert_same(device_register(INV, grid=grid), whole, "grid %d" % grid)


def test_two_runs_and_the_id_order_are_identical(whole):
    assert_same(device_register(INV), whole)
    lib = _lib.load()
    lib.gv_points_register_set_cell_order(0)                        # source points by id, not by cell
    try:
        assert_same(device_register(INV), whole, "id order")
    finally:
        lib.gv_points_register_set_cell_order(1)


def part(res, lo, hi):
    off = np.concatenate([[0], np.cumsum([len(s) for s in SOURCES])])
    out = {}
    for key in KEYS:
        if key in ("correspondence", "moved", "moved_normals"):
            out[key] = res[key][off[lo]:off[hi]]
        else:
            out[key] = res[key][lo:hi]
    return out


def test_a_pair_alone_equals_the_pair_in_the_batch(whole):
    for i, name in enumerate(ORDER):
        assert_same(device_register(INV, i, i + 1), part(whole, i, i + 1), name)


def test_a_sub_range_with_nonzero_first_offsets(whole):
    """pairs [a, b) of the packed batches through the C ABI: pointers into the packed arrays, offsets[0] != 0"""
    lib = _lib.load()
    a, b = 3, 20
    it, md, tol = INV
    src = R.PointBatch(list(zip(SOURCES, NORMALS)), DEV)
    tgt = R.PointBatch(TARGETS, DEV)
    assert src.point_offsets_host[a] != 0 and tgt.point_offsets_host[a] != 0
    s, t = src.group(a, b), tgt.group(a, b)
    n, total_s, total_t = b - a, s[3], t[3]
    ws_bytes = lib.gv_points_register_workspace_bytes(n, total_s, total_t, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    outs = dict(transforms=torch.full((n, 4, 4), 7.0, dtype=torch.float64, device=DEV),
                rmse=torch.full((n,), 7.0, dtype=torch.float64, device=DEV),
                inliers=torch.full((n,), 7, dtype=torch.int32, device=DEV),
                used=torch.full((n,), 7, dtype=torch.int32, device=DEV),
                correspondence=torch.full((total_s,), 7, dtype=torch.int32, device=DEV),
                moved=torch.full((total_s, 3), 7.0, dtype=torch.float32, device=DEV),
                moved_normals=torch.full((total_s, 3), 7.0, dtype=torch.float32, device=DEV),
                status=torch.full((n,), 7, dtype=torch.int32, device=DEV))
    init = np.ascontiguousarray(INIT[a:b])
    rc = lib.gv_points_register(s[0], s[1], t[0], t[1], n, total_s, total_t, s[4], t[4], src.group_normals(a),
                                init.ctypes.data, it, md, tol, 0, outs["transforms"].data_ptr(), outs["rmse"].data_ptr(),
                                outs["inliers"].data_ptr(), outs["used"].data_ptr(), outs["correspondence"].data_ptr(),
                                outs["moved"].data_ptr(), outs["moved_normals"].data_ptr(), ws.data_ptr(), ws_bytes,
                                outs["status"].data_ptr(), None)
    assert rc == 0
    got = {k: host(v) for k, v in outs.items()}
    want = part(whole, a, b)
    e = ORDER.index("empty_source") - a                             # nothing is written for a source without points
    assert a <= ORDER.index("empty_source") < b and got["status"][e] == EMPTY
    assert_same(got, want, "sub-range")
    # the nullable outputs may be left out, and so may the normals and the init
    again = torch.full((total_s, 3), 7.0, dtype=torch.float32, device=DEV)
    tr = torch.full((n, 4, 4), 7.0, dtype=torch.float64, device=DEV)
    rc = lib.gv_points_register(s[0], s[1], t[0], t[1], n, total_s, total_t, s[4], t[4], None, init.ctypes.data, it, md, tol,
                                0, tr.data_ptr(), None, None, None, None, again.data_ptr(), None, ws.data_ptr(), ws_bytes,
                                outs["status"].data_ptr(), None)
    assert rc == 0 and host(again).tobytes() == got["moved"].tobytes() and host(tr).tobytes() == got["transforms"].tobytes()


def test_a_permutation_of_the_target(whole):
    """targets without duplicate points: the same transforms, correspondences mapped through the permutation.  (Permuting
    the SOURCE changes the order of the sums: deliberately not asserted.)"""
    names = [k for k in ORDER if k != "coincident"]
    perms = [np.random.RandomState(70 + i).permutation(len(t)) for i, t in enumerate(TARGETS)]
    got = device_register(INV, targets=[t[p] for t, p in zip(TARGETS, perms)])       # new id j holds old point perm[j]
    off = np.concatenate([[0], np.cumsum([len(s) for s in SOURCES])])
    for name in names:
        i = ORDER.index(name)
        for key in ("transforms", "rmse", "inliers", "used", "status"):
            assert got[key][i].tobytes() == whole[key][i].tobytes(), (name, key)
        c, w = got["correspondence"][off[i]:off[i + 1]], whole["correspondence"][off[i]:off[i + 1]]
        assert (c >= 0).tolist() == (w >= 0).tolist()
        assert perms[i][c[c >= 0]].tolist() == w[w >= 0].tolist(), name
        assert got["moved"][off[i]:off[i + 1]].tobytes() == whole["moved"][off[i]:off[i + 1]].tobytes()


# ---- merged, the chain, the engine ---------------------------------------------------------------------------------------
def halves(seed):
    """two overlapping halves of one sampled box surface; the second moved by a planted transform"""
    pts = RO.box_surface(2400, (1.0, 0.6, 0.3), seed=seed)
    a, b = pts[pts[:, 0] < 0.3], pts[pts[:, 0] > -0.3]
    T = RO.rigid(RO.axis_angle((1, 2, 3), 4.0), (0.02, -0.01, 0.015))
    return a, (b.astype(D) @ T[:3, :3].T + T[:3, 3]).astype(F), T


def test_merged_is_the_pairwise_concatenation():
    rng = np.random.RandomState(0)
    sizes = [(5, 0, 3), (0, 0, 0), (300, 7, 1)]
    batches = [[rng.normal(size=(s[k], 3)).astype(F) for s in sizes] for k in range(3)]
    normals = [[rng.normal(size=c.shape).astype(F) for c in b] for b in batches]
    plain = R.PointBatch.merged(*[R.PointBatch(b, DEV) for b in batches])
    want = [np.concatenate([batches[k][m] for k in range(3)]) for m in range(3)]
    assert plain.point_offsets_host.tolist() == [0, 8, 8, 316] and plain.normals is None
    assert host(plain.point_offsets).tolist() == [0, 8, 8, 316]
    assert host(plain.points)[:316].tobytes() == np.concatenate(want).tobytes()
    withn = R.PointBatch.merged(*[R.PointBatch(list(zip(b, g)), DEV) for b, g in zip(batches, normals)])
    wantn = [np.concatenate([normals[k][m] for k in range(3)]) for m in range(3)]
    assert host(withn.normals)[:316].tobytes() == np.concatenate(wantn).tobytes()
    assert host(withn.points)[:316].tobytes() == np.concatenate(want).tobytes()
    empty = R.PointBatch.merged(R.PointBatch([np.zeros((0, 3), F)], DEV), R.PointBatch([np.zeros((0, 3), F)], DEV))
    assert empty.point_offsets_host.tolist() == [0, 0] and empty.points.shape[0] >= 1


def test_the_chain_equals_the_chain_of_oracles():
    """register -> merged -> voxel_downsample -> remove_outliers -> estimate_normals(8) -> render_points("normal")"""
    V, S = 2, 32
    fixed, moving, planted = zip(*[halves(seed) for seed in (1, 2)])
    reg = RO.register(moving, fixed, None, 30, 0.03, 0.0)
    for i in range(2):      # the planted pose is undone, up to the pull of the points just past the overlap (within 0.03)
        assert np.abs(reg["transforms"][i] @ planted[i] - np.eye(4)).max() < 2e-3, reg["transforms"][i] @ planted[i]
        assert reg["status"][i] == CONVERGED
    off = np.concatenate([[0], np.cumsum([len(m) for m in moving])])
    both = [np.concatenate([fixed[i], reg["moved"][off[i]:off[i + 1]]]) for i in range(2)]
    v = CO.voxel_downsample(both, 0.02, True)
    o = CO.remove_outliers(CO.split(v), 16, 2.0)
    want_n = NO.estimate(CO.split(o), 8, "outward")
    assert all(len(b) * 0.5 < c < len(b) * 0.95 for b, c in zip(both, v["counts"]))          # the doubled points went
    moved, transforms, info = R.PointBatch(list(moving), DEV).register(R.PointBatch(list(fixed), DEV), 30, 0.03, 0.0,
                                                                       return_info=True)
    assert host(transforms).tobytes() == reg["transforms"].tobytes() and host(info[0]).tobytes() == reg["rmse"].tobytes()
    assert moved.register_status.tolist() == reg["status"].tolist()
    merged = R.PointBatch.merged(R.PointBatch(list(fixed), DEV), moved)
    batch = merged.voxel_downsample(0.02, relative=True).remove_outliers(16, 2.0).estimate_normals(8)
    total = int(batch.point_offsets_host[-1])
    assert batch.point_offsets_host.tolist() == o["offsets"].tolist()
    assert host(batch.points)[:total].tobytes() == o["points"].tobytes()
    assert host(batch.normals)[:total].tobytes() == want_n["normals"].tobytes()
    r = R.ViewRenderer(V, S, S, device=DEV, point_reflection=dict(light="camera", two_sided=True))
    d = r.point_descriptor()
    radius = np.array([R.auto_point_radius(c, d["fit"], d["proj_scale"]) for c in o["counts"]], np.float32)
    clouds = list(zip(CO.split(o), [want_n["normals"][o["offsets"][i]:o["offsets"][i + 1]] for i in range(2)]))
    want = PO.render(clouds, d, radius, None, "normal")
    views, pid, _ = r.render_points(batch, shading="normal", return_buffers=True)
    assert host(views).tobytes() == want["f32q"].tobytes()
    assert host(pid).tobytes() == want["point_id"].tobytes() and (want["point_id"] >= 0).any()
    # the host convenience
    pts, T = R.register(moving[0], fixed[0], 30, 0.03, device=DEV)
    assert pts.tobytes() == reg["moved"][:off[1]].tobytes() and T.tobytes() == reg["transforms"][0].tobytes()


def test_the_engine_runs_on_a_merged_batch():
    N, V, S = 2, 4, 64
    fixed, moving, _ = zip(*[halves(seed) for seed in (1, 2)])
    moved = R.PointBatch(list(moving), DEV).register(R.PointBatch(list(fixed), DEV), 20, 0.03)
    merged = R.PointBatch.merged(R.PointBatch(list(fixed), DEV), moved).voxel_downsample(0.02, relative=True)
    eng = gv.GVCNN("resnet_v2_50", N, V, S, S, 10, 10, device=DEV, storage="bf16")
    eng.plan.bind(gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True))
    eng.set_head(gv.params.init_head_params(V, eng.raw.c, eng.final.c, 10, seed=3, spread_scores=True))
    r = R.ViewRenderer(V, S, S, device=DEV)
    logits = host(eng.forward_points(merged, renderer=r)[2].to(torch.float32))
    assert logits.shape[0] == N and np.isfinite(logits).all()
    assert host(eng.embed_points(merged, renderer=r)).shape[0] == N
