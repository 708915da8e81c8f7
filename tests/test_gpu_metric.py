"""GPU checks of the learned retrieval metric (csrc/metric.hip, retrieval.MetricLearner) against the fp64 reference of
tests/metric_ref.py: an integer fixture bit for bit, real-valued data within derived bounds, the update, determinism,
a synthetic problem it has to learn, and the ShapeIndex integration."""
import numpy as np
import pytest
import torch

import metric_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv():
    import gvcnn_tf_amd
    return gvcnn_tf_amd


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. exact fixture ---------------------------------------------------------------------------------------------
def exact_fixture(seed=11, n=300, d=64, r=16, classes=7):
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    w = rng.integers(-1, 2, size=(r, d)).astype(np.float32)
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    labels[rng.random(n) < 0.05] = -1
    return x, w, labels


def exact_expected(x, w, labels, b, pos_weight):
    """int64 / fp64 evaluation: every value is an integer or a multiple of 0.5, far below 2^53."""
    z = x.astype(np.int64) @ w.astype(np.int64).T
    dz, stats = ref.pair_grad_closed(z, labels, b, pos_weight)
    return z, dz, stats


def median_threshold(x, w, labels):
    z = (x.astype(np.int64) @ w.astype(np.int64).T).astype(np.float64)
    t = ref.pair_terms(z, labels, 0.0, 1.0)
    return float(int(np.median(t["d"][np.triu(t["pair"], 1)]))) + 0.5


def _exact_case(gv, x, w, labels, pos_weight=2.0):
    b = median_threshold(x, w, labels) if (labels >= 0).sum() > 1 else 0.5
    ml = gv.MetricLearner(x.shape[1], rank=w.shape[0], pos_weight=pos_weight)
    ml.load_state_dict({"W": w, "b": b})
    z, dz, stats = ml.pair_grad(x, labels)
    z_ref, dz_ref, stats_ref = exact_expected(x, w, labels, b, pos_weight)
    assert np.array_equal(_np(z).astype(np.float64), z_ref.astype(np.float64))
    assert np.array_equal(_np(dz).astype(np.float64), dz_ref)
    print("stats device %s reference %s" % (_np(stats).tolist(), stats_ref.tolist()))
    assert np.array_equal(_np(stats), stats_ref)
    return ml, stats_ref


def test_exact_fixture_bit_for_bit(gv):
    """n = 300 (ragged tiles), d = 64, r = 16, integer X and W, 7 classes and about 5 % labels -1, b = median + 0.5,
    pos_weight 2: Z, dZ_unnorm and all five statistics equal the int64 / fp64 evaluation."""
    x, w, labels = exact_fixture()
    assert (labels < 0).any()
    _, stats = _exact_case(gv, x, w, labels)
    assert 0 < stats[2] < stats[1]                               # some pairs active, some not


def test_exact_single_class(gv):
    x, w, labels = exact_fixture(seed=12, n=97)
    _exact_case(gv, x, w, np.zeros_like(labels))


@pytest.mark.parametrize("r", [130, 200])
def test_exact_wide_ranks(gv, r):
    """The 192- and 256-column forms of the pair kernel (|z| <= 64, d_ij <= 200 * 128^2 < 2^24: still exact)."""
    x, w, labels = exact_fixture(seed=14, n=150, d=32, r=r)
    _exact_case(gv, x, w, labels)


@pytest.mark.parametrize("case", ["one_row", "all_unlabelled"])
def test_no_pairs_gives_zero(gv, case):
    x, w, labels = exact_fixture(seed=13, n=1 if case == "one_row" else 70)
    if case == "all_unlabelled":
        labels[:] = -1
    ml, stats = _exact_case(gv, x, w, labels)
    assert stats[1] == 0
    loss, dw, db = ml.loss_and_grads(x, labels)
    assert float(loss) == 0.0 and float(db) == 0.0
    assert not _np(dw).any()
    before = ml.state_dict()
    ml.step(x, labels, lr=0.1)                                   # zero gradient, zero momentum: nothing moves
    after = ml.state_dict()
    assert np.array_equal(before["W"], after["W"]) and before["b"] == after["b"]


# ---- 2. real-valued pair kernel ---------------------------------------------------------------------------------------
def real_pair_fixture(seed=21, n=1000, r=128, classes=10):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    labels[rng.random(n) < 0.03] = -1
    means = rng.normal(size=(classes + 1, r)) * 0.03
    z = (means[labels] + rng.normal(size=(n, r)) / np.sqrt(r)).astype(np.float32)      # mean pair distance about 2
    return z, labels, 1.05


def ambiguous_pairs(z, labels, b, pos_weight):
    """Pairs whose fp64 hinge argument lies within tau_ij = 2e-6 (|z_i|^2 + |z_j|^2 + |b| + 1) of zero."""
    t = ref.pair_terms(z, labels, b, pos_weight)
    tau = 2e-6 * (t["sq"][:, None] + t["sq"][None, :] + abs(b) + 1.0)
    return t, t["pair"] & (np.abs(t["arg"]) <= tau)


def test_pair_kernel_real_values(gv):
    """n = 1000, r = 128, Z handed in (W = identity, so the projection is exact).  Loss within 1e-5 relative of fp64.
    Gradient, per row and component, in unnormalised units:
        |dz_dev - dz_ref| <= 1e-5 sum_j |a_ij| |z_i - z_j| + 2 sum_{j ambiguous} c_ij |z_i - z_j|
    where a pair is ambiguous when its fp64 hinge argument is within tau_ij of zero (the fp32 MFMA's error on d_ij is
    at most about 5e-7 (|z_i|^2 + |z_j|^2); tau is four times that).  Fixture conditions, checked on the reference
    alone: about a third of the pairs active; ambiguous pairs at most 0.2 % of P.  The committed seed gives
    33.6 % active pairs and 8 ambiguous pairs of 470 935 (0.0017 %)."""
    pw = 1.5
    z, labels, b = real_pair_fixture()
    b = float(np.float32(b))                                     # the value the device holds
    n, r = z.shape
    t, amb = ambiguous_pairs(z, labels, b, pw)
    up = np.triu(t["pair"], 1)
    P = int(up.sum())
    share_active = (t["active"] & up).sum() / P
    share_amb = (amb & up).sum() / P
    print("P %d active %.4f ambiguous %d (%.6f)" % (P, share_active, (amb & up).sum(), share_amb))
    assert 0.25 <= share_active <= 0.45
    assert share_amb <= 0.002

    ml = gv.MetricLearner(r, rank=r, pos_weight=pw)
    ml.load_state_dict({"W": np.eye(r, dtype=np.float32), "b": b})
    z_dev, dz_dev, stats = ml.pair_grad(z, labels)
    assert np.array_equal(_np(z_dev), z)
    stats = _np(stats)
    dz_ref, stats_ref = ref.pair_grad_closed(z, labels, b, pw)
    loss_dev, loss_ref = stats[0] / stats[1], stats_ref[0] / stats_ref[1]
    print("loss device %.9g reference %.9g" % (loss_dev, loss_ref))
    assert stats[1] == stats_ref[1]
    assert abs(loss_dev - loss_ref) <= 1e-5 * abs(loss_ref)

    z64 = z.astype(np.float64)
    bound = np.zeros((n, r))
    wa, wamb = np.abs(t["a"]), np.where(amb, t["c"], 0.0)
    for i0 in range(0, n, 50):                                   # (blocks of rows: the full tensor is n x n x r)
        diff = np.abs(z64[i0:i0 + 50, None, :] - z64[None, :, :])
        bound[i0:i0 + 50] = 1e-5 * np.einsum("ij,ijc->ic", wa[i0:i0 + 50], diff) \
            + 2.0 * np.einsum("ij,ijc->ic", wamb[i0:i0 + 50], diff)
    err = np.abs(_np(dz_dev).astype(np.float64) - dz_ref)
    print("max err / bound %.4f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


# ---- 3. projection and filter gradient -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,r", [(1000, 2048, 128), (333, 70, 40)])
def test_project_and_wgrad_against_fp64(gv, n, d, r):
    """Per element |dev - ref| <= 1e-6 (|A| |B|): the fp32 MFMA measures 3.5e-7 at K = 4096; three times that leaves
    room for the split reduction's order.  wgrad is fed the device's own dZ_unnorm and stats."""
    rng = np.random.default_rng(31 + n)
    x = rng.normal(size=(n, d)).astype(np.float32)
    labels = rng.integers(0, 8, size=n).astype(np.int64)
    ml = gv.MetricLearner(d, rank=r, seed=5)
    ml.calibrate(x, labels)
    w = _np(ml.W).astype(np.float64)
    x64 = x.astype(np.float64)
    z = _np(ml.transform(x)).astype(np.float64)
    assert z.shape == (n, r)
    err = np.abs(z - x64 @ w.T)
    assert (err <= 1e-6 * (np.abs(x64) @ np.abs(w).T)).all()

    z_dev, dz, stats = ml.pair_grad(x, labels)
    assert np.array_equal(_np(z_dev).astype(np.float64), z)
    dz, stats = _np(dz).astype(np.float64), _np(stats)
    P = stats[1]
    assert P > 0 and stats[2] > 0
    loss, dw, db = ml.loss_and_grads(x, labels)
    err = np.abs(_np(dw).astype(np.float64) - dz.T @ x64 / P)
    bound = 1e-6 * (np.abs(dz).T @ np.abs(x64)) / P
    print("wgrad max err / bound %.4f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert float(db) == np.float32(-stats[3] / P)
    assert float(loss) == np.float32(stats[0] / P)


# ---- 4. the update ------------------------------------------------------------------------------------------------
def _within_ulp(got, want64, ulps=2):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def test_step_is_the_momentum_update(gv):
    """W, b and the momentum after one step equal, within 2 ulp per element, numpy's fp32 momentum update
    m = mu m + (g + wd w), w -= lr m applied to what loss_and_grads returned for the same batch, starting from a
    non-zero momentum; the weight decay reaches W and not b.  lr, mu and wd are powers of two, so their products are
    exact and the result does not depend on which multiply-adds the device compiler fuses."""
    rng = np.random.default_rng(41)
    n, d, r = 400, 256, 32
    x = rng.normal(size=(n, d)).astype(np.float32)
    labels = rng.integers(0, 6, size=n).astype(np.int64)
    f = np.float32
    lr, mu, wd = f(0.125), f(0.5), f(2.0 ** -7)
    ml = gv.MetricLearner(d, rank=r, seed=2)
    ml.calibrate(x, labels)
    s0 = ml.state_dict()
    s0["momentum_W"] = (rng.normal(size=(r, d)) * 0.01).astype(np.float32)
    s0["momentum_b"] = f(-0.25)
    ml.load_state_dict(s0)
    loss, dw, db = ml.loss_and_grads(x, labels)
    dw, db = _np(dw), f(float(db))
    assert np.abs(dw).max() > 0 and db != 0
    ml.step(x, labels, float(lr), mu=float(mu), weight_decay=float(wd))
    s1 = ml.state_dict()
    m_w = mu * s0["momentum_W"] + (dw + wd * s0["W"])
    w1 = s0["W"] - lr * m_w
    m_b = mu * s0["momentum_b"] + db
    b1 = s0["b"] - lr * m_b
    assert m_w.dtype == np.float32 and w1.dtype == np.float32
    assert _within_ulp(s1["momentum_W"], m_w.astype(np.float64)).all()
    assert _within_ulp(s1["W"], w1.astype(np.float64)).all()
    assert _within_ulp(np.asarray(s1["momentum_b"]), np.asarray(m_b, dtype=np.float64)).all()
    assert _within_ulp(np.asarray(s1["b"]), np.asarray(b1, dtype=np.float64)).all()
    assert abs(lr * wd * s0["b"]) > 100 * np.spacing(b1)         # decay on b would have shown
    assert np.abs(wd * s0["W"]).max() > 100 * np.spacing(np.abs(m_w).max())      # and its absence on W


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
def test_fit_is_deterministic(gv):
    rng = np.random.default_rng(51)
    n, d = 2000, 256
    labels = rng.integers(0, 12, size=n).astype(np.int64)
    x = (rng.normal(size=(12, d))[labels] * 0.5 + rng.normal(size=(n, d))).astype(np.float32)
    runs = []
    for _ in range(2):
        ml = gv.MetricLearner(d, rank=64, seed=3)
        hist = ml.fit(x, labels, steps=20, batch=512, lr=0.05)
        s = ml.state_dict()
        runs.append((s["W"], s["b"], hist))
    assert runs[0][2].shape == (20,) and np.isfinite(runs[0][2]).all()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2])
    assert not np.array_equal(runs[0][0], ref.init_w(d, 64, 3))


# ---- 6. it learns -------------------------------------------------------------------------------------------------------
LEARN_LR, LEARN_STEPS, LEARN_RANK = 0.05, 200, 16


def learn_fixture(seed=61, classes=10, per_class=40, d=256, d_signal=8, d_noise=56):
    """Descriptors whose class structure lives in an 8-dimensional subspace (class means and within-class noise there)
    under much larger label-free noise in 56 further dimensions, the whole rotated by a seeded orthogonal matrix.
    Returns (train x, train labels, test x, test labels): a seeded half each."""
    rng = np.random.default_rng(seed)
    n = classes * per_class
    labels = np.repeat(np.arange(classes), per_class).astype(np.int64)
    u = np.zeros((n, d))
    u[:, :d_signal] = rng.normal(size=(classes, d_signal))[labels] + 0.5 * rng.normal(size=(n, d_signal))
    u[:, d_signal:d_signal + d_noise] = 1.5 * rng.normal(size=(n, d_noise))
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    x = (u @ q.T).astype(np.float32)
    order = rng.permutation(n)
    tr, te = order[:n // 2], order[n // 2:]
    return x[tr], labels[tr], x[te], labels[te]


def learn_reference(seed):
    """(mAP of the raw test descriptors, mAP after the fp64 reference fit) for one fixture seed."""
    xtr, ltr, xte, lte = learn_fixture(seed)
    w, _, hist = ref.fit(xtr, ltr, ref.init_w(xtr.shape[1], LEARN_RANK, 0), LEARN_STEPS, LEARN_LR)
    return ref.self_map(xte, lte), ref.self_map(xte.astype(np.float64) @ w.T, lte), hist


def test_it_learns(gv):
    """10 classes x 40 shapes, d = 256, fit on a seeded half, leave-one-out mAP on the other half, r = 16, 200
    full-batch steps.  The same problem is fitted by tests/metric_ref.py in fp64 at run time: gain_ref =
    mAP_ref_learned - mAP_raw must be >= 0.15 (a property of the fixture: the committed seed 61 gives 0.435 — raw 0.185,
    learned 0.619 — and its neighbours 60 and 62 give 0.620 and 0.605).  The device loss history has to end below half
    its first value, and mAP_dev_learned >= mAP_raw + 0.5 gain_ref: device and reference trajectories part ways at the first pair that flips and no bound on
    their distance can be derived, so the margin only separates "learns as the reference does" from "does not"."""
    xtr, ltr, xte, lte = learn_fixture()
    map_raw, map_ref, hist_ref = learn_reference(61)
    gain_ref = map_ref - map_raw
    print("mAP raw %.4f reference learned %.4f gain %.4f" % (map_raw, map_ref, gain_ref))
    assert gain_ref >= 0.15

    ml = gv.MetricLearner(xtr.shape[1], rank=LEARN_RANK, seed=0)
    hist = ml.fit(xtr, ltr, steps=LEARN_STEPS, lr=LEARN_LR)
    print("loss first %.5f last %.5f (reference %.5f -> %.5f)" % (hist[0], hist[-1], hist_ref[0], hist_ref[-1]))
    assert hist[-1] < 0.5 * hist[0]
    idx = gv.ShapeIndex(xtr.shape[1], projection=ml)
    idx.add(xte, lte)
    map_dev = idx.self_map()
    raw = gv.ShapeIndex(xtr.shape[1])
    raw.add(xte, lte)
    print("mAP device learned %.4f, device raw %.4f" % (map_dev, raw.self_map()))
    assert abs(raw.self_map() - map_raw) < 1e-3
    assert map_dev >= map_raw + 0.5 * gain_ref


# ---- 7. index integration -------------------------------------------------------------------------------------------------
def test_index_with_projection(gv):
    rng = np.random.default_rng(71)
    n, d, r = 500, 200, 48
    labels = rng.integers(0, 9, size=n).astype(np.int64)
    x = (rng.normal(size=(9, d))[labels] + rng.normal(size=(n, d))).astype(np.float32)
    ml = gv.MetricLearner(d, rank=r, seed=4)
    ml.fit(x, labels, steps=5, lr=0.05)
    z = ml.transform(x)
    assert tuple(z.shape) == (n, r) and z.is_contiguous()

    a = gv.ShapeIndex(d, projection=ml)
    a.add(x[:300], labels[:300]).add(x[300:], labels[300:])
    b = gv.ShapeIndex(r)
    b.add(z, labels)
    assert len(a) == len(b) == n and a.dim == r
    da, ia = a.search(x[:64], k=10)
    db_, ib = b.search(z[:64], k=10)
    assert torch.equal(ia, ib) and torch.equal(da, db_)
    apa = a.average_precision(x[:64], labels[:64])
    apb = b.average_precision(z[:64], labels[:64])
    assert torch.equal(apa, apb)
    assert torch.equal(a.self_average_precision(), b.self_average_precision())
    with pytest.raises(ValueError):
        a.add(_np(z), labels)                                    # projected rows where raw descriptors are expected

    other = gv.MetricLearner(d, rank=r, seed=99)
    assert not torch.equal(other.transform(x), z)
    other.load_state_dict(ml.state_dict())
    assert torch.equal(other.transform(x), z)
    s = ml.state_dict()
    assert isinstance(s["W"], np.ndarray) and s["W"].shape == (r, d) and s["W"].dtype == np.float32
