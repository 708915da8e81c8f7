"""Cleaning on the device against the numpy restatement of its contract (tests/points_clean_oracle.py), byte for byte in
keep, kept points, index, mean distances, stats, counts and status; invariance under the grid hint, batching, a
sub-range of a batch, repetition and point order; normals carried along; the chain downsample -> remove outliers ->
estimate normals -> render against the chain of oracles; the engine on a cleaned batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib, render as R         # noqa: E402

import point_normals_oracle as NO                  # noqa: E402
import points_clean_oracle as CO                   # noqa: E402
import render_points_oracle as PO                  # noqa: E402
from test_gpu_point_normals import BASE            # noqa: E402  (the named clouds)

DEV = torch.device("cuda:0")
F = np.float32
PASS = _lib.GV_POINTS_CLEAN_PASSTHROUGH


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def planted(P, n_out, seed):
    rng = np.random.RandomState(seed)
    inliers = unit(rng.normal(size=(P, 3)))
    far = unit(rng.normal(size=(n_out, 3))) * rng.uniform(4.0, 8.0, size=(n_out, 1))
    return np.concatenate([inliers, far]).astype(F)


# ---- clouds ------------------------------------------------------------------------------------------------------------
def sized(n, seed):
    return np.random.RandomState(seed).normal(size=(n, 3)).astype(F)


# the block edges of the tree sum and of the scan (256 values a block), and two levels of the tree
EDGES = {"n255": sized(255, 1), "n256": sized(256, 2), "n257": sized(257, 3), "n1025": sized(1025, 4)}
ORDER = ["one", "two", "three", "km1", "coincident", "k", "empty", "collinear", "lattice", "kp1", "flat", "kp2", "crowd",
         "sphere", "n255", "n256", "n257", "n1025", "surface"]    # the empty cloud sits in the middle
_tables = {}


def clouds_for(k):
    """([points], [key table with 32 columns]) of the batch for k: the named clouds, the block-edge sizes and clouds of
    k - 1 .. k + 2 points.  A table is computed once per cloud; the k smallest keys are its first k columns."""
    named = dict(BASE, **EDGES)
    named.update(km1=sized(k - 1, 100 + k), k=sized(k, 200 + k), kp1=sized(k + 1, 300 + k), kp2=sized(k + 2, 400 + k))
    out, tables = [], []
    for name in ORDER:
        key = name if name in BASE or name in EDGES else (name, k)
        if key not in _tables:
            _tables[key] = CO.key_table(named[name], 32)
        out.append(named[name])
        tables.append(_tables[key])
    return out, tables


def keep_of(index, new_offsets, old_offsets):
    keep = np.zeros(int(old_offsets[-1]), np.int32)
    for i in range(len(old_offsets) - 1):
        keep[old_offsets[i] + index[new_offsets[i]:new_offsets[i + 1]].astype(np.int64)] = 1
    return keep


def collect(batch, new, index):
    total = int(new.point_offsets_host[-1])
    out = {"points": host(new.points)[:total], "index": host(index)[:total],
           "counts": np.diff(new.point_offsets_host).astype(np.int32), "offsets": host(new.point_offsets),
           "status": new.clean_status.copy(),
           "normals": None if new.normals is None else host(new.normals)[:total]}
    assert out["offsets"].tolist() == new.point_offsets_host.tolist()
    return out


def device_outliers(clouds, k, ratio, grid=None):
    batch = R.PointBatch(clouds, DEV)
    new, index, (md, stats) = batch.remove_outliers(k, ratio, grid, return_index=True, return_stats=True)
    total = int(batch.point_offsets_host[-1])
    out = collect(batch, new, index)
    out.update(mean_dist=host(md)[:total], stats=host(stats),
               keep=keep_of(out["index"], out["offsets"], batch.point_offsets_host))
    return out


def device_voxels(clouds, voxel, relative):
    batch = R.PointBatch(clouds, DEV)
    new, index = batch.voxel_downsample(voxel, relative, return_index=True)
    return collect(batch, new, index)


OUTLIER_KEYS = ("keep", "points", "index", "mean_dist", "stats", "counts", "offsets", "status")
VOXEL_KEYS = ("points", "index", "counts", "offsets", "status")


def assert_same(got, want, keys, what=""):
    for key in keys:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), "%s %s: %d entries differ" % (what, key, (g != w).sum())


# ---- the device against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("k", [1, 8, 16, 17, 32])
def test_outlier_removal_equals_oracle(k, ratio):
    clouds, tables = clouds_for(k)
    want = CO.remove_outliers(clouds, k, ratio, tables=tables)
    got = device_outliers(clouds, k, ratio)
    assert_same(got, want, OUTLIER_KEYS)
    st = dict(zip(ORDER, got["status"].tolist()))
    none = ("empty", "km1") if k == 1 else ("empty",)              # k - 1 = 0 points
    assert all(v == (_lib.GV_RENDER_EMPTY if n in none else 0) for n, v in st.items()), st
    cnt = dict(zip(ORDER, got["counts"].tolist()))
    assert cnt["empty"] == 0 and cnt["one"] == 1 and cnt["coincident"] >= 4
    if ratio == 2.0 and k >= 8:
        i = ORDER.index("crowd")                                    # 1 500 points in a ball and one far away
        kept = got["index"][got["offsets"][i]:got["offsets"][i + 1]]
        assert 1500 not in kept.tolist() and len(kept) >= 1400


_large = {}


def large_clouds():
    """A cloud needs more than 65 536 points before level 1 of the tree sum has a second block and level 2 reads more
    than one partial: 65 536 (one full level-1 block) and 65 537 (one value into the second), behind a small cloud so that
    their first point is no multiple of 256.  Line clouds: the k = 1 table in O(P) (CO.line_key_table)."""
    if not _large:
        small = sized(300, 9)
        lines = [CO.line_cloud(65536, 21), CO.line_cloud(65537, 22)]
        _large["clouds"] = [small] + [pts for pts, _ in lines]
        tables = [CO.key_table(small, 1)] + [CO.line_key_table(pts, perm) for pts, perm in lines]
        _large["want"] = CO.remove_outliers(_large["clouds"], 1, 1.0, tables=tables)
    return _large["clouds"], _large["want"]


@pytest.mark.parametrize("grid", [None, 128])
def test_outlier_removal_past_65536_points_equals_oracle(grid):
    """the third level of the tree sum, and the scan and the gather past 256 blocks of a cloud"""
    clouds, want = large_clouds()
    got = device_outliers(clouds, 1, 1.0, grid=grid)
    assert_same(got, want, OUTLIER_KEYS, "grid %s" % grid)
    assert got["status"].tolist() == [0, 0, 0]
    assert all(0.5 * len(c) < n < len(c) for c, n in zip(clouds, got["counts"].tolist()))       # some go, most stay


VOXELS = {"rel_0.05": (0.05, True), "rel_0.25": (0.25, True), "rel_1.0": (1.0, True), "abs_0.3": (0.3, False),
          "per_cloud": (None, True)}


@pytest.mark.parametrize("name", sorted(VOXELS))
def test_voxel_downsampling_equals_oracle(name):
    clouds, _ = clouds_for(16)
    voxel, relative = VOXELS[name]
    if voxel is None:
        voxel = np.random.RandomState(8).uniform(0.03, 0.6, size=len(clouds)).astype(F)
    want = CO.voxel_downsample(clouds, voxel, relative)
    got = device_voxels(clouds, voxel, relative)
    assert_same(got, want, VOXEL_KEYS, name)
    st = dict(zip(ORDER, got["status"].tolist()))
    cnt = dict(zip(ORDER, got["counts"].tolist()))
    assert st["empty"] == _lib.GV_RENDER_EMPTY and cnt["empty"] == 0
    if relative:                                                    # relative to no extent: h = 0, passthrough
        assert st["one"] == PASS and cnt["one"] == 1
    else:
        assert st["one"] == 0 and cnt["one"] == 1
    assert st["surface"] == 0 and 1 <= cnt["surface"] < 5000
    if name == "rel_1.0":                                           # cells 0 and 1 on the longest axis only
        assert all(c <= 8 for n, c in cnt.items() if st[n] == 0)


def test_selection_arrays_through_the_c_abi_equal_oracle():
    """keep / centroids / index before the compaction, on a sub-range with point_offsets[0] != 0, for both selections;
    and the compaction of that sub-range"""
    k = 16
    clouds, tables = clouds_for(k)
    batch = R.PointBatch(clouds, DEV)
    lib = _lib.load()
    a, b = 4, 18
    po = batch.point_offsets_host
    assert po[a] != 0
    args = batch.group(a, b)
    n, total = args[2], args[3]
    ws_bytes = lib.gv_points_clean_workspace_bytes(n, total, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)        # noqa: E731
    f32 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)    # noqa: E731
    keep, md, status = i32(total), f32(total), i32(n)
    stats = torch.full((n, 3), 7.0, dtype=torch.float64, device=DEV)
    rc = lib.gv_points_outlier_select(*args, k, 2.0, 0, keep.data_ptr(), md.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                      ws_bytes, status.data_ptr(), None)
    assert rc == 0
    want = CO.remove_outliers(clouds[a:b], k, 2.0, tables=tables[a:b])
    got = {"keep": host(keep), "mean_dist": host(md), "stats": host(stats), "status": host(status)}
    assert_same(got, want, ("keep", "mean_dist", "stats", "status"))
    outs = dict(points=f32(total, 3), index=i32(total), offsets=torch.full((n + 1,), 7, dtype=torch.int64, device=DEV),
                counts=i32(n))

    def compact(keep, selected, index):
        rc = lib.gv_points_compact(*args, keep.data_ptr(), selected, index, None, status.data_ptr(),
                                   outs["points"].data_ptr(), None, outs["index"].data_ptr(), outs["offsets"].data_ptr(),
                                   outs["counts"].data_ptr(), ws.data_ptr(), ws_bytes, None)
        assert rc == 0
        got = {key: host(t) for key, t in outs.items()}
        new_total = int(got["offsets"][-1])
        got["points"], got["index"] = got["points"][:new_total], got["index"][:new_total]
        return got
    assert_same(compact(keep, None, None), want, ("points", "index", "offsets", "counts"))
    # the nullable outputs may be left out
    again = i32(total)
    rc = lib.gv_points_outlier_select(*args, k, 2.0, 0, again.data_ptr(), None, None, ws.data_ptr(), ws_bytes,
                                      status.data_ptr(), None)
    assert rc == 0 and host(again).tobytes() == got["keep"].tobytes()
    # voxel selection
    voxel = np.full(n, 0.25, F)
    cen, index = f32(total, 3), i32(total)
    rc = lib.gv_points_voxel_select(*args, voxel.ctypes.data, 1, 0, keep.data_ptr(), cen.data_ptr(), index.data_ptr(),
                                    ws.data_ptr(), ws_bytes, status.data_ptr(), None)
    assert rc == 0
    want = CO.voxel_downsample(clouds[a:b], 0.25, True)
    got = {"keep": host(keep), "centroids": host(cen), "index_all": host(index), "status": host(status)}
    assert_same(got, want, ("keep", "centroids", "index_all", "status"))
    assert_same(compact(keep, cen.data_ptr(), index.data_ptr()), want, ("points", "index", "offsets", "counts"))


# ---- invariance -------------------------------------------------------------------------------------------------------
K_INV = 16


@pytest.fixture(scope="module")
def whole():
    clouds, _ = clouds_for(K_INV)
    return clouds, device_outliers(clouds, K_INV, 2.0), device_voxels(clouds, 0.25, True)


@pytest.mark.parametrize("grid", [1, 7, 128])
def test_the_grid_hint_changes_nothing(whole, grid):
    """grid = 1 is brute force on the device; 128 is clamped per cloud (None is the fixture's)"""
    clouds, first, _ = whole
    assert_same(device_outliers(clouds, K_INV, 2.0, grid=grid), first, OUTLIER_KEYS, "grid %d" % grid)


def test_two_runs_are_identical(whole):
    clouds, first, firstv = whole
    assert_same(device_outliers(clouds, K_INV, 2.0), first, OUTLIER_KEYS)
    assert_same(device_voxels(clouds, 0.25, True), firstv, VOXEL_KEYS)


def test_a_cloud_alone_equals_the_cloud_in_the_batch(whole):
    clouds, first, firstv = whole
    old = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])

    def part(res, i, keys):
        o = res["offsets"]
        out = {}
        for key in keys:
            if key in ("points", "index"):
                out[key] = res[key][o[i]:o[i + 1]]
            elif key in ("keep", "mean_dist"):
                out[key] = res[key][old[i]:old[i + 1]]
            elif key == "offsets":
                out[key] = np.array([0, o[i + 1] - o[i]], np.int64)
            else:
                out[key] = res[key][i:i + 1]
        return out
    for i, c in enumerate(clouds):
        assert_same(device_outliers([c], K_INV, 2.0), part(first, i, OUTLIER_KEYS), OUTLIER_KEYS, ORDER[i])
        assert_same(device_voxels([c], 0.25, True), part(firstv, i, VOXEL_KEYS), VOXEL_KEYS, ORDER[i])


def test_a_permutation_of_the_points():
    """no two distances tie on this cloud, so ids never decide: the same points are kept, with the same mean distances;
    the voxels' centroids are the same set (integer sums know no order), and each representative maps through the
    permutation"""
    pts = planted(1000, 5, 6)
    perm = np.random.RandomState(5).permutation(len(pts))           # new id t holds old point perm[t]
    a, b = device_outliers([pts], K_INV, 2.0), device_outliers([pts[perm]], K_INV, 2.0)
    assert sorted(perm[b["index"]].tolist()) == a["index"].tolist() and 900 < len(a["index"]) <= 1000
    assert b["mean_dist"].tobytes() == a["mean_dist"][perm].tobytes()
    a, b = device_voxels([pts], 0.1, False), device_voxels([pts[perm]], 0.1, False)
    rows_a = sorted(zip(a["points"].view(np.uint32).tolist(), a["index"].tolist()))
    rows_b = sorted(zip(b["points"].view(np.uint32).tolist(), perm[b["index"]].tolist()))
    assert rows_a == rows_b and len(rows_a) > 50


# ---- normals, chaining, the engine --------------------------------------------------------------------------------------
def test_normals_are_carried_along():
    clouds = [planted(700, 6, 3), BASE["lattice"], BASE["flat"]]
    rng = np.random.RandomState(2)
    normals = [rng.normal(size=c.shape).astype(F) for c in clouds]
    batch = R.PointBatch(list(zip(clouds, normals)), DEV)
    batch.normal_status = np.array([0, 0x100, 0], np.int32)
    for new, index, want in (
            batch.remove_outliers(8, 1.0, return_index=True) + (CO.remove_outliers(clouds, 8, 1.0, normals=normals),),
            batch.voxel_downsample(0.2, True, return_index=True) + (CO.voxel_downsample(clouds, 0.2, True, normals=normals),)):
        got = collect(batch, new, index)
        assert_same(got, want, ("points", "index", "normals", "counts"))
        flat = np.concatenate(normals)
        src = np.concatenate([batch.point_offsets_host[i] + got["index"][got["offsets"][i]:got["offsets"][i + 1]]
                              for i in range(3)])
        assert got["normals"].tobytes() == flat[src].tobytes()      # out_normals == normals[index]
    assert batch.remove_outliers(8, 1.0).normal_status.tolist() == [0, 0x100, 0]
    assert batch.voxel_downsample(0.2, True).normal_status is None
    # from_device: a batch from device tensors feeds the same calls
    again = R.PointBatch.from_device(batch.points, batch.point_offsets_host, batch.normals)
    new, index = again.remove_outliers(8, 1.0, return_index=True)
    assert_same(collect(again, new, index), CO.remove_outliers(clouds, 8, 1.0, normals=normals),
                ("points", "index", "normals", "counts"))


def test_the_chain_equals_the_chain_of_oracles():
    """voxel_downsample -> remove_outliers -> estimate_normals(8) -> render_points(shading="normal")"""
    V, S = 2, 32
    pts = planted(2000, 10, 2)
    v = CO.voxel_downsample([pts], 0.1, False)
    o = CO.remove_outliers([v["points"]], 16, 2.0)
    want_n = NO.estimate([o["points"]], 8, "outward")
    assert 500 < len(o["points"]) == len(v["points"]) - 10 and np.abs(o["points"]).max() < 1.5      # the far points went
    batch = R.PointBatch([pts], DEV).voxel_downsample(0.1).remove_outliers(16, 2.0).estimate_normals(8)
    total = int(batch.point_offsets_host[-1])
    assert host(batch.points)[:total].tobytes() == o["points"].tobytes()
    assert host(batch.normals)[:total].tobytes() == want_n["normals"].tobytes()
    r = R.ViewRenderer(V, S, S, device=DEV, point_reflection=dict(light="camera", two_sided=True))
    d = r.point_descriptor()
    radius = np.array([R.auto_point_radius(total, d["fit"], d["proj_scale"])], np.float32)
    want = PO.render([(o["points"], want_n["normals"])], d, radius, None, "normal")
    views, pid, _ = r.render_points(batch, shading="normal", return_buffers=True)
    assert host(views).tobytes() == want["f32q"].tobytes()
    assert host(pid).tobytes() == want["point_id"].tobytes() and (want["point_id"] >= 0).any()
    # the host conveniences
    kept, index = R.remove_outliers(v["points"], 16, 2.0, device=DEV)
    assert kept.tobytes() == o["points"].tobytes() and index.tobytes() == o["index"].tobytes()
    cen, index = R.voxel_downsample(pts, 0.1, device=DEV)
    assert cen.tobytes() == v["points"].tobytes() and index.tobytes() == v["index"].tobytes()


def test_the_engine_sees_the_clean_cloud():
    """forward_points on the planted cloud after remove_outliers against the 2 000 clean points alone: the bound is 1e-5
    relative; the kept points ARE the clean points, so the logits are the same bytes (the equality
    tests/test_gpu_render_points.py asks of the engine on equal views)"""
    N, V, S = 2, 4, 64
    dirty = [planted(2000, 10, 2), planted(2000, 10, 3)]
    clean = [c[:2000] for c in dirty]
    eng = gv.GVCNN("resnet_v2_50", N, V, S, S, 10, 10, device=DEV, storage="bf16")
    eng.plan.bind(gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True))
    eng.set_head(gv.params.init_head_params(V, eng.raw.c, eng.final.c, 10, seed=3, spread_scores=True))
    r = R.ViewRenderer(V, S, S, device=DEV)
    cleaned = R.PointBatch(dirty, DEV).remove_outliers(16, 2.0)
    assert cleaned.num_points.tolist() == [2000, 2000]
    got = host(eng.forward_points(cleaned, renderer=r)[2].to(torch.float32)).copy()
    want = host(eng.forward_points(R.PointBatch(clean, DEV), renderer=r)[2].to(torch.float32)).copy()
    spoilt = host(eng.forward_points(R.PointBatch(dirty, DEV), renderer=r)[2].to(torch.float32)).copy()
    assert np.isfinite(want).all() and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert got.tobytes() == want.tobytes()
    assert spoilt.tobytes() != want.tobytes()                       # the outliers did shrink the object
    assert host(eng.embed_points(cleaned, renderer=r)).shape[0] == N


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_statuses_only_the_c_abi_can_reach():
    """a cloud with a NaN point passes through with GV_RENDER_NONFINITE | GV_POINTS_CLEAN_PASSTHROUGH, one whose offsets
    run backwards is GV_RENDER_BAD_OFFSETS with a count of 0, and the clouds around them are cleaned as ever"""
    lib = _lib.load()
    good = BASE["sphere"]
    nan = BASE["flat"][:50].copy()
    nan[7, 1] = np.nan
    allp = np.concatenate([good, nan, good])
    pts = torch.from_numpy(allp).to(DEV)
    P, Q = len(good), len(nan)
    n, total, k = 4, 2 * P + Q, 8
    offs = torch.tensor([0, P, P + Q, total, total - 3], dtype=torch.int64, device=DEV)      # the last cloud: backwards
    ws_bytes = lib.gv_points_clean_workspace_bytes(n, total, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    keep = torch.full((total,), 7, dtype=torch.int32, device=DEV)
    cen = torch.full((total, 3), 7.0, dtype=torch.float32, device=DEV)
    index = torch.full((total,), 7, dtype=torch.int32, device=DEV)
    status = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    out_p = torch.full((total, 3), 7.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((total,), 7, dtype=torch.int32, device=DEV)
    out_o = torch.full((n + 1,), 7, dtype=torch.int64, device=DEV)
    counts = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    want_status = [0, _lib.GV_RENDER_NONFINITE | PASS, 0, _lib.GV_RENDER_BAD_OFFSETS]
    wo = CO.remove_outliers([good], k, 2.0)
    wv = CO.voxel_downsample([good], 0.25, True)
    voxel = np.full(n, 0.25, F)
    for which, want in (("outliers", wo), ("voxels", wv)):
        if which == "outliers":
            rc = lib.gv_points_outlier_select(pts.data_ptr(), offs.data_ptr(), n, total, P, k, 2.0, 0, keep.data_ptr(), None,
                                              None, ws.data_ptr(), ws_bytes, status.data_ptr(), None)
            sel = (None, None)
        else:
            rc = lib.gv_points_voxel_select(pts.data_ptr(), offs.data_ptr(), n, total, P, voxel.ctypes.data, 1, 0,
                                            keep.data_ptr(), cen.data_ptr(), index.data_ptr(), ws.data_ptr(), ws_bytes,
                                            status.data_ptr(), None)
            sel = (cen.data_ptr(), index.data_ptr())
        assert rc == 0 and host(status).tolist() == want_status, which
        assert (host(keep)[P:P + Q] == 1).all()
        rc = lib.gv_points_compact(pts.data_ptr(), offs.data_ptr(), n, total, P, keep.data_ptr(), sel[0], sel[1], None,
                                   status.data_ptr(), out_p.data_ptr(), None, out_i.data_ptr(), out_o.data_ptr(),
                                   counts.data_ptr(), ws.data_ptr(), ws_bytes, None)
        assert rc == 0
        c = int(want["counts"][0])
        assert host(counts).tolist() == [c, Q, c, 0] and host(out_o).tolist() == [0, c, c + Q, 2 * c + Q, 2 * c + Q]
        got_p, got_i = host(out_p), host(out_i)
        for a in (0, c + Q):                                        # the sphere, before and after the NaN cloud
            assert got_p[a:a + c].tobytes() == want["points"].tobytes() and got_i[a:a + c].tobytes() == want["index"].tobytes()
        assert got_p[c:c + Q].tobytes() == nan.tobytes() and got_i[c:c + Q].tolist() == list(range(Q))


def test_every_error_clause_leaves_the_outputs_alone():
    lib = _lib.load()
    pts = torch.from_numpy(BASE["sphere"]).to(DEV)
    P, n = len(BASE["sphere"]), 1
    offs = torch.tensor([0, P], dtype=torch.int64, device=DEV)
    ws_bytes = lib.gv_points_clean_workspace_bytes(n, P, 0)
    ws = torch.full((ws_bytes + 16,), 7, dtype=torch.uint8, device=DEV)
    bufs = {name: torch.full(shape, 7, dtype=dt, device=DEV) for name, shape, dt in (
        ("keep", (P,), torch.int32), ("md", (P,), torch.float32), ("stats", (n, 3), torch.float64),
        ("status", (n,), torch.int32), ("cen", (P, 3), torch.float32), ("index", (P,), torch.int32),
        ("out_p", (P, 3), torch.float32), ("out_i", (P,), torch.int32), ("out_o", (n + 1,), torch.int64),
        ("counts", (n,), torch.int32))}
    p = {name: t.data_ptr() for name, t in bufs.items()}
    voxel = np.full(n, 0.25, F)
    BADARG, UNSUPPORTED, ALIGN = _lib.GV_E_BADARG, _lib.GV_E_UNSUPPORTED, _lib.GV_E_ALIGN

    def outliers(n=n, k=8, ratio=2.0, grid=0, w=ws.data_ptr(), wb=ws_bytes, mp=P, keep=p["keep"]):
        return lib.gv_points_outlier_select(pts.data_ptr(), offs.data_ptr(), n, P, mp, k, ratio, grid, keep, p["md"],
                                            p["stats"], w, wb, p["status"], None)

    def voxels(n=n, relative=1, grid=0, w=ws.data_ptr(), wb=ws_bytes, mp=P, v=voxel.ctypes.data, cen=p["cen"]):
        return lib.gv_points_voxel_select(pts.data_ptr(), offs.data_ptr(), n, P, mp, v, relative, grid, p["keep"], cen,
                                          p["index"], w, wb, p["status"], None)

    def compact(n=n, w=ws.data_ptr(), wb=ws_bytes, mp=P, counts=p["counts"], out_o=p["out_o"]):
        return lib.gv_points_compact(pts.data_ptr(), offs.data_ptr(), n, P, mp, p["keep"], None, None, None, p["status"],
                                     p["out_p"], None, p["out_i"], out_o, counts, w, wb, None)
    for f in (outliers, voxels, compact):
        assert f(n=0) == BADARG and f(wb=16) == BADARG and f(mp=-1) == BADARG
        assert f(n=65536) == UNSUPPORTED and f(mp=(1 << 24) + 1) == UNSUPPORTED
        assert f(w=ws.data_ptr() + 8) == ALIGN
    assert outliers(k=0) == BADARG and outliers(k=33) == BADARG and outliers(ratio=-1.0) == BADARG
    assert outliers(ratio=float("nan")) == BADARG and outliers(grid=129) == BADARG and outliers(keep=None) == BADARG
    assert outliers(keep=p["keep"] + 2) == ALIGN
    assert voxels(relative=2) == BADARG and voxels(v=None) == BADARG and voxels(grid=-1) == BADARG
    assert voxels(cen=p["cen"] + 1) == ALIGN
    assert compact(counts=None) == BADARG and compact(out_o=p["out_o"] + 4) == ALIGN
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert (t == 7).all().item(), name
    assert (ws == 7).all().item()
