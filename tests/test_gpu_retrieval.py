"""Shape retrieval on the device against a numpy oracle (float64 / int64, np.lexsort on (id, distance)).

Integer-valued descriptors in [-3, 3] make every dot product, norm and distance an integer below 2^24: exact in fp32,
bf16 and fp16 storage alike, so ids AND distances must equal the oracle bit for bit, ties ordered by id included.
Real-valued data is checked against the oracle's distance of each returned id within the stated tolerances."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import retrieval as R            # noqa: E402

DEV = "cuda:0"
STORAGES = ["f32", "bf16", "f16"]
TORCH16 = {"bf16": torch.bfloat16, "f16": torch.float16}


# ---- oracle --------------------------------------------------------------------------------------------------------
def oracle_l2(q, x):
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return np.maximum(0.0, (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * q @ x.T)


def oracle_cosine(q, x):
    def unit(a):
        a = np.asarray(a, np.float64)
        n = np.sqrt((a * a).sum(1, keepdims=True))
        return np.divide(a, n, out=np.zeros_like(a), where=n > 0)
    return 1.0 - unit(q) @ unit(x).T


def oracle_order(D, exclude=None):
    """[nq, ndb] ranking of every query: ascending distance, equal distances by the lower id (excluded rows last)."""
    D = np.array(D, np.float64, copy=True)
    if exclude is not None:
        for i, e in enumerate(exclude):
            if 0 <= e < D.shape[1]:
                D[i, e] = np.inf
    ids = np.broadcast_to(np.arange(D.shape[1]), D.shape)
    return np.lexsort((ids, D), axis=-1), D


def oracle_topk(D, k, exclude=None):
    order, Dx = oracle_order(D, exclude)
    nq, ndb = D.shape
    n_valid = ndb - (0 if exclude is None else np.array([(0 <= e < ndb) for e in exclude], np.int64))
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float64)
    m = min(k, ndb)
    ids[:, :m] = order[:, :m]
    dist[:, :m] = np.take_along_axis(Dx, order[:, :m], 1)
    for i in range(nq):
        nv = int(n_valid if np.isscalar(n_valid) else n_valid[i])
        ids[i, nv:], dist[i, nv:] = -1, np.inf
    return dist, ids


def oracle_ap(D, q_labels, db_labels, exclude=None):
    order, _ = oracle_order(D, exclude)
    db_labels = np.asarray(db_labels)
    out = np.full(D.shape[0], np.nan)
    for i in range(D.shape[0]):
        if q_labels[i] < 0:
            continue
        o = order[i]
        if exclude is not None and 0 <= exclude[i] < D.shape[1]:
            o = o[o != exclude[i]]
        rel = db_labels[o] == q_labels[i]
        r = int(rel.sum())
        if r:
            out[i] = np.sum(np.arange(1, r + 1) / (np.nonzero(rel)[0] + 1)) / r
    return out


def ints(shape, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float32)


def exact_data(nq, ndb, d, seed):
    """Integer descriptors with duplicated rows, queries equal to stored rows (distance-0 ties with the duplicates) and
    rows one unit away (distances that differ by 1)."""
    rng = np.random.default_rng(seed)
    x = ints((ndb, d), seed)
    q = ints((nq, d), seed + 1)
    src = rng.choice(ndb, 40, replace=False)
    x[rng.choice(ndb, 40, replace=False)] = x[src]                    # duplicated rows
    q[:20] = x[src[:20]]                                               # queries with (several) exact matches
    for j in range(20, 30):                                            # neighbours at distance 1, 2, ... of a query
        for t in range(4):
            r = (7 * j + 131 * t) % ndb
            x[r] = q[j]
            x[r, t] = x[r, t] + (1 if x[r, t] < 3 else -1)
    return q, x


def host(t):
    return t.cpu().numpy()


# ---- 1. exact search -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2048, 100])
def test_exact_search_equals_oracle(d):
    nq, ndb = 257, 4099
    q, x = exact_data(nq, ndb, d, seed=d)
    D = oracle_l2(q, x)
    assert D.max() < 2 ** 24
    ex = np.arange(nq)
    want = {k: oracle_topk(D, k) for k in (1, 10, 256)}
    want_ex = oracle_topk(D, 10, exclude=ex)
    for storage in STORAGES:
        idx = R.ShapeIndex(d, "l2", storage, device=DEV).add(torch.from_numpy(x))
        assert len(idx) == ndb
        qd = torch.from_numpy(q).to(DEV)
        for k, (od, oi) in want.items():
            dist, ids = idx.search(qd, k)
            np.testing.assert_array_equal(host(ids), oi, err_msg="%s k=%d" % (storage, k))
            np.testing.assert_array_equal(host(dist), od.astype(np.float32), err_msg="%s k=%d" % (storage, k))
        dist, ids = idx.search(qd, 10, exclude=torch.from_numpy(ex))              # leave-self-out
        np.testing.assert_array_equal(host(ids), want_ex[1], err_msg=storage)
        np.testing.assert_array_equal(host(dist), want_ex[0].astype(np.float32), err_msg=storage)


def test_exact_search_chunking_is_bitwise_neutral():
    nq, ndb, d = 257, 4099, 2048
    q, x = exact_data(nq, ndb, d, seed=5)
    D = oracle_l2(q, x)
    for storage in STORAGES:
        idx = R.ShapeIndex(d, "l2", storage, device=DEV).add(torch.from_numpy(x))
        qd = torch.from_numpy(q).to(DEV)
        d0, i0 = idx.search(qd, 256)
        d1, i1 = idx.search(qd, 256, db_chunk=256)
        d2, i2 = idx.search(qd, 256, db_chunk=1280, exclude=np.arange(nq))
        assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), storage
        od, oi = oracle_topk(D, 256, exclude=np.arange(nq))
        np.testing.assert_array_equal(host(i2), oi)
        np.testing.assert_array_equal(host(d2), od.astype(np.float32))


def test_search_pads_short_databases():
    x = ints((5, 100), 11)
    q = ints((3, 100), 12)
    for storage in STORAGES:
        idx = R.ShapeIndex(100, "l2", storage, device=DEV).add(x)
        dist, ids = idx.search(q, 10)
        od, oi = oracle_topk(oracle_l2(q, x), 10)
        np.testing.assert_array_equal(host(ids), oi)
        np.testing.assert_array_equal(host(dist), od.astype(np.float32))
        assert (host(ids)[:, 5:] == -1).all() and np.isposinf(host(dist)[:, 5:]).all()
        dist, ids = idx.search(q, 10, exclude=[0, 4, 99])                  # 99: out of range, excludes nothing
        assert (host(ids)[:2, 4:] == -1).all() and (host(ids)[2, :5] >= 0).all()
        assert 0 not in host(ids)[0] and 4 not in host(ids)[1]


# ---- 2. real-valued search -----------------------------------------------------------------------------------------
def round16(a, storage):
    return torch.from_numpy(a).to(TORCH16[storage]).to(torch.float32).numpy() if storage in TORCH16 else a


@pytest.mark.parametrize("storage,metric", [("f32", "l2"), ("f32", "cosine"), ("bf16", "l2"), ("f16", "l2"),
                                            ("bf16", "cosine"), ("f16", "cosine")])
def test_real_valued_search(storage, metric):
    rng = np.random.default_rng(3)
    nq, ndb, d, k = 100, 2000, 2048, 32
    x = rng.standard_normal((ndb, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    x[7] = 0.0                                                              # a zero row (cosine: stays zero)
    idx = R.ShapeIndex(d, metric, storage, device=DEV).add(x)
    dist, ids = idx.search(q, k)
    dist, ids = host(dist).astype(np.float64), host(ids)
    if metric == "l2":
        qr, xr = round16(q, storage), round16(x, storage)
        D = oracle_l2(qr, xr)
        tol = 1e-5 * ((qr.astype(np.float64) ** 2).sum(1)[:, None] + (xr.astype(np.float64) ** 2).sum(1)[None, :])
    else:
        D = oracle_cosine(q, x)
        tol = np.full(D.shape, 1e-5 if storage == "f32" else 2e-2)
    rows = np.arange(nq)[:, None]
    assert (ids >= 0).all()
    np.testing.assert_array_less(np.abs(dist - D[rows, ids]), tol[rows, ids] + 1e-12)
    kth = np.sort(D, 1)[:, k - 1]
    assert (np.abs(dist[:, -1] - kth) <= tol[rows[:, 0], ids[:, -1]] + 1e-12).all()
    for i in range(nq):
        assert len(set(ids[i].tolist())) == k
    order_ok = (dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (ids[:, 1:] > ids[:, :-1]))
    assert order_ok.all()


# ---- 3. exact AP ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,n,d", [("f32", 600, 2048), ("bf16", 600, 2048), ("f16", 1100, 100)])
def test_exact_average_precision(storage, n, d):
    rng = np.random.default_rng(n + d)
    x = ints((n, d), n)
    x[rng.choice(n, 30, replace=False)] = x[rng.choice(n, 30, replace=False)]      # duplicates: distance ties
    labels = rng.integers(0, 40, n)
    labels[rng.choice(n, 25, replace=False)] = -1                                  # unlabelled rows
    labels[3] = 99                                                                 # a class of one: NaN left out
    idx = R.ShapeIndex(d, "l2", storage, device=DEV).add(x, torch.from_numpy(labels))
    D = oracle_l2(x, x)
    ex = np.arange(n)
    want = oracle_ap(D, labels, labels, ex)
    assert np.isnan(want[3]) and np.isnan(want).sum() >= 25
    got = host(idx.average_precision(x, labels, exclude=ex))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=1e-6)
    self_ap = host(idx.self_average_precision())
    assert self_ap.tobytes() == got.tobytes()
    assert idx.self_map() == pytest.approx(float(np.nanmean(got.astype(np.float64))), abs=1e-12)
    assert idx.mean_average_precision(x, labels, exclude=ex) == pytest.approx(float(np.nanmean(want)), abs=1e-6)


def test_average_precision_at_the_database_cap():
    n, d, nq = R.AP_MAX_DB, 64, 6
    x = ints((n, d), 21)
    labels = np.random.default_rng(22).integers(0, 40, n)
    q = x[:nq].copy()
    idx = R.ShapeIndex(d, "l2", "bf16", device=DEV).add(x, labels)
    want = oracle_ap(oracle_l2(q, x), labels[:nq], labels, np.arange(nq))
    got = host(idx.average_precision(q, labels[:nq], exclude=np.arange(nq)))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    idx.add(x[:1], labels[:1])
    with pytest.raises(gv._lib.GvError) as e:
        idx.average_precision(q, labels[:nq])
    assert e.value.code == gv._lib.GV_E_UNSUPPORTED


# ---- 4. search and AP agree ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric", [("f32", "l2"), ("bf16", "cosine")])
def test_search_and_average_precision_agree(storage, metric):
    rng = np.random.default_rng(8)
    n, d = 200, 256
    x = rng.standard_normal((n, d)).astype(np.float32)
    labels = rng.integers(0, 5, n)
    labels[:3] = -1
    idx = R.ShapeIndex(d, metric, storage, device=DEV).add(x, labels)
    ex = np.arange(n)
    _, ids = idx.search(x, n, exclude=ex)
    ids = host(ids)
    want = np.full(n, np.nan)
    for i in range(n):
        if labels[i] < 0:
            continue
        ranked = ids[i][ids[i] >= 0]
        assert len(ranked) == n - 1
        rel = labels[ranked] == labels[i]
        r = int(rel.sum())
        if r:
            want[i] = np.sum(np.arange(1, r + 1) / (np.nonzero(rel)[0] + 1)) / r
    got = host(idx.average_precision(x, labels, exclude=ex))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=1e-6)


# ---- 5. determinism ------------------------------------------------------------------------------------------------
def test_search_and_average_precision_are_deterministic():
    rng = np.random.default_rng(13)
    x = rng.standard_normal((3000, 2048)).astype(np.float32)
    labels = rng.integers(0, 40, 3000)
    for storage in ("f32", "bf16"):
        idx = R.ShapeIndex(2048, "l2", storage, device=DEV).add(x, labels)
        a = [idx.search(x[:300], 100, db_chunk=1024) for _ in range(2)]
        assert host(a[0][0]).tobytes() == host(a[1][0]).tobytes()
        assert host(a[0][1]).tobytes() == host(a[1][1]).tobytes()
        b = [host(idx.self_average_precision()) for _ in range(2)]
        assert b[0].tobytes() == b[1].tobytes()


# ---- 6. end to end -------------------------------------------------------------------------------------------------
def make_engine(backbone, N, V, H, W, C, G, **kw):
    eng = gv.GVCNN(backbone, N, V, H, W, C, G, device=DEV, **kw)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C, seed=3, spread_scores=True)
    eng.plan.bind(P)
    eng.set_head(Hd)
    return eng


def views(N, V, H, W, seed):
    return torch.rand(N, V, H, W, 3, generator=torch.Generator().manual_seed(seed)) - 0.5


def test_embed_and_retrieval_evaluator_end_to_end():
    eng = make_engine("resnet_v2_50", 2, 3, 64, 64, 10, 10)
    x = views(2, 3, 64, 64, 0).to(DEV)
    e = eng.embed(x)
    assert e.shape == (2, eng.final.c) and e.dtype == torch.float32
    assert torch.equal(e, eng.gap) and e.data_ptr() != eng.gap.data_ptr()
    eb = eng.embed(x, basic=True)
    assert torch.equal(eb, eng.gap)

    ev = R.RetrievalEvaluator(eng)
    batches = [(views(2, 3, 64, 64, 1), [0, 1], None), (views(2, 3, 64, 64, 2), [1, 0], None),
               (views(2, 3, 64, 64, 3), [0, -1], 1)]                       # last batch padded: one real shape
    emb, labs = [], []
    for v, lab, valid in batches:
        ev.add_batch(v.to(DEV), torch.tensor(lab), valid=valid)
        nv = 2 if valid is None else valid
        emb.append(host(eng.gap)[:nv].astype(np.float64))
        labs += lab[:nv]
    mAP, ap, num = ev.result()
    assert num == 5 and ap.shape == (5,)
    E, L = np.concatenate(emb), np.array(labs)
    want = oracle_ap(oracle_l2(E, E), L, L, np.arange(5))
    np.testing.assert_array_equal(np.isnan(ap), np.isnan(want))
    np.testing.assert_allclose(ap[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-6)
    assert math.isclose(mAP, float(np.nanmean(want)), abs_tol=1e-6)
