"""tests/head_ref.py (the reference of the grouping-head sweep, tests/test_gpu_head.py) against oracle/grouping.py and the
golden grouping vectors, at the small geometries of the sweep.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import grouping as OG
import head_ref as HR

F32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of fp32
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grouping_golden.json")))


def _scores(case):
    return np.array([np.frombuffer(bytes.fromhex(h), dtype=np.float32)[0] for h in case["scores_f32_hex"]], dtype=np.float32)


@pytest.mark.parametrize("N,V,hw,cr", [(3, 4, 16, 32), (1, 1, 1, 30), (3, 5, 49, 8)])
@pytest.mark.parametrize("order", [HR.SHAPE_MAJOR, HR.VIEW_MAJOR])
def test_score_against_the_oracle(N, V, hw, cr, order):
    """r_img, batch mean and closed-form score against oracle view_score (per view; it rounds the pooled map, r and the
    score to fp32): |d score| <= |dr| / (1 + r)^2 + (|ln r| + 3) u score with |dr| <= u (sum |gap k| + |r|), u = 2^-24 — the
    first two roundings, and a term that also covers an fp32 evaluation of sigmoid(log r)."""
    g = torch.Generator().manual_seed(N * 100 + V * 10 + order)
    raw5 = torch.randn(N, V, hw, cr, generator=g)                                   # [n, v, p, c]
    kern, bias = torch.randn(V, cr, generator=g) * 0.3, torch.randn(V, generator=g)
    raw = (raw5 if order == HR.SHAPE_MAJOR else raw5.permute(1, 0, 2, 3)).reshape(N * V, hw, cr)
    r_img, sabs = HR.score_partial(raw, kern, bias, V, order)
    for b in range(N * V):
        n, v = (b // V, b % V) if order == HR.SHAPE_MAJOR else (b % N, b // N)
        want = (raw5[n, v].double() * kern[v].double()).sum() / hw + bias[v].double()
        assert abs(float(r_img[b] - want)) <= 1e-12 * float(sabs[b] / hw + abs(bias[v]))
    score, r, _ = HR.view_score(r_img, N, V, order)
    for v in range(V):
        o = float(OG.view_score(raw5[:, v].reshape(N, hw, 1, cr).numpy(), kern[v].numpy(), float(bias[v])))
        gap = raw5[:, v].double().mean(1)
        rv = abs(float(r[v]))
        dr = U * (float((gap.abs() @ kern[v].double().abs()).mean()) + rv + abs(float(bias[v])))
        tol = dr / (1 + max(rv - dr, 0.0)) ** 2 + (abs(np.log(rv)) + 3) * U * float(score[v])
        assert abs(o - float(score[v])) <= tol, (v, o, float(score[v]), tol)


def _grid():
    return np.exp(np.linspace(np.log(1e-6), np.log(1e6), 20001)).astype(F32)


def test_closed_form_score_within_one_ulp_of_score_from_r():
    """|r| / (1 + |r|) against oracle score_from_r (sigmoid(log|r|), fp64 inside, rounded once) on r in [1e-6, 1e6]: one fp32
    ulp of the score.  (An fp32 evaluation of sigmoid(log r) cannot meet this: the rounding of ln r to fp32 alone moved the
    oracle's earlier fp32 form up to 9.4 ulp from the closed form on this grid, at r = 7.25e-6.)"""
    r = _grid()
    got = HR.score_closed(torch.from_numpy(r)).numpy()
    o = OG.score_from_r(r)
    ulps = np.abs(o.astype(np.float64) - got) / np.spacing(got.astype(F32)).astype(np.float64)
    i = int(ulps.argmax())
    print("closed form vs score_from_r: worst %.2f ulp at r = %.4e" % (ulps[i], r[i]))
    assert o.dtype == F32 and ulps.max() <= 1.0, "worst %.2f ulp at r = %.4e" % (ulps[i], r[i])


def test_closed_form_score_at_the_special_values():
    special = HR.score_closed(torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), -3.0, 1e-40],
                                           dtype=torch.float64)).numpy()
    assert special[:4].tolist() == [0.0, 0.0, 1.0, 1.0] and np.isnan(special[4]) and special[5] == 0.75
    assert special[6] == 1e-40 / (1 + 1e-40)
    o = OG.score_from_r(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -3.0], F32))
    assert o[:4].tolist() == [0.0, 0.0, 1.0, 1.0] and np.isnan(o[4]) and o[5] == F32(0.75) and OG.score_from_r(F32(0)) == 0.0


@pytest.mark.parametrize("V,N,G,E", [(6, 2, 5, 48), (5, 1, 10, 3), (20, 2, 10, 27)])
@pytest.mark.parametrize("mode,fill", [("max", 1.0), ("mean", 0.0)])
def test_pool_and_fuse_against_the_oracle(V, N, G, E, mode, fill):
    """fp64 pooling == oracle view_pooling on float64 input to 1e-12 (max: equal); the ordered fp32 restatement ==
    view_pooling + group_fusion on float32 input bit for bit (the oracle adds in the same order); fp64 fusion within
    (G + 2) 2^-23 sum_g |w_g D_g| / wsum of it (G additions, the product, the division)."""
    rng = np.random.RandomState(V * 7 + N)
    F = rng.randn(N, V, E).astype(F32)
    scheme = OG.group_scheme([rng.uniform(0, G / 10.0 - 1e-3, size=V).astype(F32)], G, V)
    weight = OG.group_weight(scheme)
    D64, S64 = HR.pool_fuse(torch.from_numpy(F), scheme, weight, mode, fill)
    o64 = OG.view_pooling([F[:, v].astype(np.float64) for v in range(V)], scheme, pool=mode, empty_fill=fill)
    o32 = OG.view_pooling([F[:, v] for v in range(V)], scheme, pool=mode, empty_fill=fill)
    oS = OG.group_fusion(o32, weight)
    D32, S32 = HR.pool_fuse_f32(F, scheme, weight, mode, fill)
    for g in range(G):
        assert np.abs(D64[g].numpy() - o64[g]).max() <= 1e-12 * max(1.0, np.abs(o64[g]).max())
        assert np.array_equal(D32[g], o32[g])
    assert np.array_equal(S32, oS)
    sabs = sum(abs(float(weight[g])) * np.abs(D64[g].numpy()) for g in range(G)) / float(weight.sum())
    assert (np.abs(S64.numpy() - oS) <= (G + 2) * 2.0 ** -23 * sabs + (V + 1) * U * sabs).all()


def test_gap_dense_and_metrics_against_the_oracle():
    """global_average_pool and dense of the oracle accumulate in fp64 and round once: half an fp32 ulp of the result."""
    rng = np.random.RandomState(5)
    x = rng.randn(3, 7, 7, 20).astype(F32)
    m, sabs = HR.global_avg_pool(torch.from_numpy(x).reshape(3, 49, 20))
    assert (np.abs(OG.global_average_pool(x) - m.numpy()) <= U * np.abs(m.numpy()) + 1e-300).all()
    assert np.allclose(sabs.numpy(), np.abs(x.astype(np.float64)).sum((1, 2)), rtol=1e-12)
    a, k, b = rng.randn(5, 24).astype(F32), rng.randn(24, 40).astype(F32), rng.randn(40).astype(F32)
    y, yabs = HR.dense(torch.from_numpy(a), torch.from_numpy(k), torch.from_numpy(b))
    assert (np.abs(OG.dense(a, k, b) - y.numpy()) <= U * np.abs(y.numpy()) + 1e-12 * yabs.numpy()).all()
    yy, bound = HR.scale_shift_act(torch.from_numpy(a), torch.from_numpy(k[:, 0]), torch.from_numpy(b[:24]), 1)
    assert np.array_equal(yy.numpy(), np.maximum(a.astype(np.float64) * k[:, 0] + b[:24].astype(np.float64), 0))
    assert (bound.numpy() >= np.abs(yy.numpy())).all()
    logits = rng.randint(-2, 3, size=(50, 4)).astype(F32)                       # many ties
    labels = rng.randint(-1, 6, size=50)
    pred, conf, corr = HR.eval_metrics(logits, labels, np.ones((4, 4), np.int64), 3)
    want = np.ones((4, 4), np.int64)
    n_ok = 3
    for i in range(50):
        p = [j for j in range(4) if logits[i, j] == logits[i].max()][0]
        assert pred[i] == p
        if 0 <= labels[i] < 4:
            want[labels[i], p] += 1
            n_ok += int(labels[i] == p)
    assert conf.tolist() == want.tolist() and corr == n_ok


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_ordered_group_assign_against_the_golden_vectors(case):
    s = _scores(case)
    gidx, scheme, weight, status = HR.group_assign_f32(s, case["G"], 10)
    if case["error"] == "IndexError":
        assert status & 1
        return
    assert status == 0 and scheme.tolist() == case["scheme"] and weight.tolist() == case["weight"]
    assert gidx.tolist() == OG.group_index(s).tolist()
    assert scheme.tolist() == OG.group_scheme([s], case["G"], case["V"]).tolist()


def test_ordered_fusion_reproduces_kat1_bit_for_bit():
    k = GOLD["kat1"]
    F = np.array(k["final_view_descriptors"], dtype=F32)[None]                  # [N = 1, V = 5, E = 4]
    sch = np.array(k["group_scheme"])
    D, S = HR.pool_fuse_f32(F, sch, np.array(k["model_py_weight"], F32), "max", 1.0)
    for g, exp in k["model_py_group_max"].items():
        assert D[int(g), 0].tolist() == exp
    want = np.array(k["model_py_shape_descriptor"], dtype=F32)
    assert S.dtype == F32 and S[0].tobytes() == want.tobytes()
    Dm, _ = HR.pool_fuse(torch.from_numpy(F), sch, np.array(k["model_py_weight"], F32), "mean", 0.0)
    for g, exp in k["unit_test_mean_int32"].items():                            # unit_test.py: int32 mean truncates
        assert np.trunc(Dm[int(g), 0].numpy()).tolist() == exp


@pytest.mark.parametrize("weight_mode", ["count", "mean_score"])
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_ordered_per_shape_grouping_against_the_oracle(weight_mode, pool):
    """Scores from responses, per-shape schemes, both weight modes and the fused descriptor, bit for bit against
    per_shape_grouping (it is built from the same fp32 operations); shape 3 has r = 0: weights 0 under mean-score, S = 0."""
    rng = np.random.RandomState(11)
    N, V, G, E = 5, 7, 10, 12
    r = rng.uniform(-8.0, 8.0, size=(N, V)).astype(F32)
    r[3] = 0.0
    F = rng.randn(N, V, 1, 1, E).astype(F32)
    scores, schemes, weights, S = OG.per_shape_grouping(F, r, G, 10, weight_mode, pool, 1.0)
    closed = HR.view_score_per_shape(torch.from_numpy(r)).numpy()
    assert (np.abs(scores - closed) <= (np.abs(np.log(np.maximum(np.abs(r), 1e-30))) + 4) * U * closed).all()
    gidx, sch, w, status = HR.group_assign_per_shape_f32(scores, G, 10, weight_mode)
    assert status == 0 and sch.tolist() == schemes.tolist() and w.tobytes() == weights.astype(F32).tobytes()
    _, S32 = HR.pool_fuse_f32(F.reshape(N, V, E), sch, w, pool, 1.0)
    assert S32.tobytes() == S.reshape(N, E).astype(F32).tobytes()
    D64, S64 = HR.pool_fuse(torch.from_numpy(F.reshape(N, V, E)), sch, w, pool, 1.0)
    sabs = (np.abs(w.T[:, :, None].astype(np.float64)) * np.abs(D64.numpy())).sum(0)
    wsum = np.abs(w.astype(np.float64).sum(1))[:, None]
    assert (np.abs(S64.numpy() - S32) * np.maximum(wsum, 1e-300) <= (2 * G + V + 3) * 2.0 ** -23 * sabs).all()
    if weight_mode == "mean_score":
        assert float(np.abs(w[3]).sum()) == 0.0 and float(S64[3].abs().max()) == 0.0


def test_group_assign_status_cases():
    gidx, scheme, weight, status = HR.group_assign_f32([0.1, float("nan"), 1.0, -0.5, 0.999], 10, 10)
    assert gidx.tolist() == [1, -1, 10, -5, 9] and status == 3
    assert scheme.sum(0).tolist() == [1, 0, 0, 0, 1] and weight.tolist() == [1, 2, 1, 1, 1, 1, 1, 1, 1, 2]
    _, _, w, _ = HR.group_assign_f32([0.11, 0.15, 0.95], 10, 10, "mean_score")
    assert w[1] == F32(F32(F32(0.11) + F32(0.15)) / F32(2)) and w[9] == F32(0.95) and w[0] == 0
