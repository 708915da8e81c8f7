"""Normal estimation on the device against the numpy restatement of its contract (tests/point_normals_oracle.py), byte for
byte in normals, neighbours, variation and status; invariance under the grid hint, batching, a sub-range of a batch,
repetition and point order; the renders and the engine on an estimated batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib, render as R         # noqa: E402

import point_normals_oracle as NO                  # noqa: E402
import render_points_oracle as PO                  # noqa: E402

DEV = torch.device("cuda:0")
F = np.float32
KEYS = ("normals", "neighbours", "variation", "status")
DEGENERATE = _lib.GV_POINTS_DEGENERATE_NORMAL


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- clouds --------------------------------------------------------------------------------------------------------
def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def base_clouds():
    """every cloud the contract has a clause for that does not depend on k, by name"""
    rng = np.random.RandomState(11)
    g = np.arange(6, dtype=np.float64)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    verts, tris = R.icosphere(2)
    flat = rng.uniform(-1, 1, size=(400, 3))
    flat[:, 2] = 0.0
    return {
        "one": np.array([(0.5, 0.5, 0.5)], F),
        "two": np.array([(0.3, -0.2, 0.1), (-0.4, 0.5, -0.6)], F),
        "three": np.array([(0.3, -0.2, 0.1), (-0.4, 0.5, -0.6), (0.9, 0.1, 0.2)], F),
        "empty": np.zeros((0, 3), F),
        "coincident": np.array([(0.2, 0.2, 0.2)] * 4 + [(-0.7, -0.1, 0.4)], F),
        "collinear": np.stack([np.arange(8) * 0.25, np.arange(8) * 0.5, np.arange(8) * -0.125], axis=1).astype(F),
        "lattice": np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F),       # exact distance ties everywhere
        "flat": flat.astype(F),                                                        # no extent along z
        "crowd": np.concatenate([rng.uniform(-1, 1, size=(1500, 3)) * 0.12 / np.sqrt(3.0), [(1.0, 1.0, 1.0)]]).astype(F),
        "sphere": unit(rng.normal(size=(300, 3))),                                     # no distance ties
        "surface": R.sample_surface(verts, tris, 5000, seed=2)[0],
    }


BASE = base_clouds()
ORDER = ["one", "two", "three", "below", "coincident", "at", "empty", "collinear", "lattice", "above", "flat", "crowd",
         "sphere", "surface"]                                     # the empty cloud sits in the middle
_nb = {}


def clouds_for(k):
    """([points], [neighbour table with 32 columns]) of the batch for k: the base clouds and three of k - 1, k and k + 1
    points.  The tables are computed once per cloud; the k smallest keys are their first k columns."""
    rng = np.random.RandomState(100 + k)
    named = dict(BASE, below=rng.normal(size=(k - 1, 3)).astype(F), at=rng.normal(size=(k, 3)).astype(F),
                 above=rng.normal(size=(k + 1, 3)).astype(F))
    out, nbs = [], []
    for name in ORDER:
        key = name if name in BASE else (name, k)
        if key not in _nb:
            _nb[key] = NO.neighbours(named[name], 32)
        out.append(named[name])
        nbs.append(_nb[key])
    return out, nbs


# the viewpoint outside every cloud, and inside the large ones (the surface cloud is a unit sphere around the origin)
ORIENTS = {"none": ("none", None), "outward": ("outward", None), "view_outside": ("viewpoint", (3.0, -4.0, 5.0)),
           "view_inside": ("viewpoint", (0.05, -0.02, 0.1))}


def device_estimate(clouds, k, orient="outward", viewpoint=None, grid=None):
    batch = R.PointBatch(clouds, DEV)
    _, nb, var = batch.estimate_normals(k, orient, viewpoint, grid, return_neighbors=True, return_variation=True)
    total = int(batch.point_offsets_host[-1])
    return {"normals": host(batch.normals)[:total], "neighbours": host(nb)[:total], "variation": host(var)[:total],
            "status": batch.normal_status.copy()}


def assert_same(got, want, what=""):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert got[key].tobytes() == want[key].tobytes(), \
            "%s %s: %d entries differ" % (what, key, (got[key] != want[key]).sum())


# ---- the device against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("orient", sorted(ORIENTS))
@pytest.mark.parametrize("k", [3, 8, 16, 17, 32])
def test_device_equals_oracle(k, orient):
    clouds, nbs = clouds_for(k)
    mode, vp = ORIENTS[orient]
    want = NO.estimate(clouds, k, mode, vp, nbs)
    got = device_estimate(clouds, k, mode, vp)
    assert_same(got, want)
    st = dict(zip(ORDER, want["status"].tolist()))
    assert st["empty"] == _lib.GV_RENDER_EMPTY
    for name in ("one", "two", "coincident", "collinear"):
        assert st[name] == DEGENERATE, name
    for name in ("three", "flat", "sphere", "surface", "above"):
        assert st[name] == 0, name
    # the neighbourhoods hold what the clause says: -1 past P, the point itself first among distinct points
    po = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    two = got["neighbours"][po[1]:po[2]]
    assert two[:, :2].tolist() == [[0, 1], [1, 0]] and (two[:, 2:] == -1).all()
    sph = got["neighbours"][po[12]:po[13]]
    assert (sph[:, 0] == np.arange(300)).all() and (sph >= 0).all()
    n = got["normals"][po[12]:po[13]].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)


# ---- invariance -------------------------------------------------------------------------------------------------------
K_INV = 16


@pytest.fixture(scope="module")
def whole():
    clouds, _ = clouds_for(K_INV)
    return clouds, device_estimate(clouds, K_INV, "outward")


@pytest.mark.parametrize("grid", [1, 2, 7, 128])
def test_the_grid_hint_changes_nothing(whole, grid):
    """grid = 1 is brute force on the device; 128 is clamped per cloud"""
    clouds, first = whole
    assert_same(device_estimate(clouds, K_INV, "outward", grid=grid), first, "grid %d" % grid)


def test_two_runs_are_identical(whole):
    clouds, first = whole
    assert_same(device_estimate(clouds, K_INV, "outward"), first)


def test_a_cloud_alone_equals_the_cloud_in_the_batch(whole):
    clouds, first = whole
    po = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    for i, c in enumerate(clouds):
        one = device_estimate([c], K_INV, "outward")
        part = {"normals": first["normals"][po[i]:po[i + 1]], "neighbours": first["neighbours"][po[i]:po[i + 1]],
                "variation": first["variation"][po[i]:po[i + 1]], "status": first["status"][i:i + 1]}
        assert_same(one, part, ORDER[i])


def test_a_sub_range_with_a_nonzero_first_offset(whole):
    """clouds [a, b) of the packed batch through the C ABI: pointers into the packed arrays, offsets[0] != 0"""
    clouds, first = whole
    batch = R.PointBatch(clouds, DEV)
    lib = _lib.load()
    a, b = 4, 13
    po = batch.point_offsets_host
    assert po[a] != 0
    args = batch.group(a, b)
    n, total = args[2], args[3]
    ws_bytes = lib.gv_points_normals_workspace_bytes(n, total, 0)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    normals = torch.full((total, 3), 7.0, dtype=torch.float32, device=DEV)
    nb = torch.full((total, K_INV), 7, dtype=torch.int32, device=DEV)
    var = torch.full((total,), 7.0, dtype=torch.float32, device=DEV)
    status = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    rc = lib.gv_points_estimate_normals(*args, K_INV, _lib.GV_NORMALS_ORIENT_OUTWARD, None, 0, normals.data_ptr(),
                                        nb.data_ptr(), var.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(), None)
    assert rc == 0
    got = {"normals": host(normals), "neighbours": host(nb), "variation": host(var), "status": host(status)}
    part = {"normals": first["normals"][po[a]:po[b]], "neighbours": first["neighbours"][po[a]:po[b]],
            "variation": first["variation"][po[a]:po[b]], "status": first["status"][a:b]}
    assert_same(got, part)
    # the nullable outputs may be left out
    again = torch.empty_like(normals)
    rc = lib.gv_points_estimate_normals(*args, K_INV, _lib.GV_NORMALS_ORIENT_OUTWARD, None, 0, again.data_ptr(), None,
                                        None, ws.data_ptr(), ws_bytes, status.data_ptr(), None)
    assert rc == 0 and host(again).tobytes() == got["normals"].tobytes()


def test_a_permutation_of_the_points_permutes_the_normals():
    pts = BASE["sphere"]                                               # no two distances tie: ids never decide
    perm = np.random.RandomState(5).permutation(len(pts))
    for orient, vp in (("outward", None), ("viewpoint", (3.0, -4.0, 5.0))):
        a = device_estimate([pts], K_INV, orient, vp)
        b = device_estimate([pts[perm]], K_INV, orient, vp)
        assert b["normals"].tobytes() == a["normals"][perm].tobytes()
        assert b["variation"].tobytes() == a["variation"][perm].tobytes()
        assert (perm[b["neighbours"]] == a["neighbours"][perm]).all()


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_render_and_engine_on_an_estimated_batch():
    V, S = 4, 64
    clouds = [BASE["surface"], BASE["flat"], BASE["coincident"]]       # the last one's normals are all zero: depth factor
    want_n = NO.estimate(clouds, K_INV, "outward")
    r = R.ViewRenderer(V, S, S, device=DEV, point_reflection=dict(light="camera", two_sided=True))
    batch = R.PointBatch(clouds, DEV, estimate_normals=K_INV)
    assert batch.normal_status.tolist() == want_n["status"].tolist() == [0, 0, DEGENERATE]
    d = r.point_descriptor()
    radius = np.array([R.auto_point_radius(len(c), d["fit"], d["proj_scale"]) for c in clouds], np.float32)
    po = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    with_normals = [(c, want_n["normals"][po[i]:po[i + 1]]) for i, c in enumerate(clouds)]
    want = PO.render(with_normals, d, radius, None, "normal")
    views, pid, depth = r.render_points(batch, shading="normal", return_buffers=True)
    assert host(views).tobytes() == want["f32q"].tobytes()
    assert host(pid).tobytes() == want["point_id"].tobytes()
    assert host(r.render_points_uint8(batch, shading="normal")).tobytes() == want["u8"].tobytes()
    assert (want["point_id"][:2] >= 0).any()
    # without an estimate the existing error stays
    with pytest.raises(ValueError, match="needs a batch with normals"):
        r.render_points(R.PointBatch(clouds, DEV), shading="normal")
    # the engine takes the batch as it takes any other
    N = 2
    eng = gv.GVCNN("resnet_v2_50", N, V, S, S, 10, 10, device=DEV, storage="bf16")
    eng.plan.bind(gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True))
    eng.set_head(gv.params.init_head_params(V, eng.raw.c, eng.final.c, 10, seed=3, spread_scores=True))
    two = R.PointBatch(clouds[:N], DEV).estimate_normals(K_INV)
    assert isinstance(two, R.PointBatch)
    logits = host(eng.forward_points(two, renderer=r, shading="normal")[2].to(torch.float32))
    assert logits.shape == (N, 10) and np.isfinite(logits).all()
    # the convenience for one host cloud
    one = R.estimate_normals(clouds[0], K_INV, device=DEV)
    assert one.tobytes() == want_n["normals"][:po[1]].tobytes()


def test_statuses_only_the_c_abi_can_reach():
    """PointBatch refuses non-finite points and builds its own offsets; through the C ABI a cloud with a NaN point is
    GV_RENDER_NONFINITE (zero normals, -1 neighbours, variation 0) and one whose offsets run backwards is
    GV_RENDER_BAD_OFFSETS (nothing is written for it), while the clouds around them are estimated as ever."""
    lib = _lib.load()
    good = BASE["sphere"]
    nan = BASE["flat"][:50].copy()
    nan[7, 1] = np.nan
    pts = torch.from_numpy(np.concatenate([good, nan, good])).to(DEV)
    P, Q = len(good), len(nan)
    n, total, k = 4, 2 * P + Q, 8
    offs = torch.tensor([0, P, P + Q, total, total - 3], dtype=torch.int64, device=DEV)      # the last cloud: backwards
    ws_bytes = lib.gv_points_normals_workspace_bytes(n, total, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    normals = torch.full((total, 3), 7.0, dtype=torch.float32, device=DEV)
    nb = torch.full((total, k), 7, dtype=torch.int32, device=DEV)
    var = torch.full((total,), 7.0, dtype=torch.float32, device=DEV)
    status = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    rc = lib.gv_points_estimate_normals(pts.data_ptr(), offs.data_ptr(), n, total, P, k, _lib.GV_NORMALS_ORIENT_NONE,
                                        None, 0, normals.data_ptr(), nb.data_ptr(), var.data_ptr(), ws.data_ptr(),
                                        ws_bytes, status.data_ptr(), None)
    assert rc == 0
    assert host(status).tolist() == [0, _lib.GV_RENDER_NONFINITE, 0, _lib.GV_RENDER_BAD_OFFSETS]
    got_n, got_nb, got_var = host(normals), host(nb), host(var)
    want = NO.estimate_cloud(good, k, "none")
    for a in (0, P + Q):                                               # the sphere, before and after the NaN cloud
        assert got_n[a:a + P].tobytes() == want["normals"].tobytes()
        assert got_nb[a:a + P].tobytes() == want["neighbours"].tobytes()
        assert got_var[a:a + P].tobytes() == want["variation"].tobytes()
    assert (got_n[P:P + Q] == 0).all() and (got_nb[P:P + Q] == -1).all() and (got_var[P:P + Q] == 0).all()
