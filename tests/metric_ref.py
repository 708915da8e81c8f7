"""CPU reference of the learned retrieval metric (helper, not collected): the objective of include/gvcnn_hip.h
("learned retrieval metric") twice — in torch fp64 with autograd, and as a closed-form numpy gradient — plus the
fp64 training loop and the leave-one-out mAP that test_gpu_metric.py compares the device with.

    z_i = W x_i,  d_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j),  pairs i < j with both labels >= 0 (P of them),
    y_ij = +1 (equal labels) / -1,  c_ij = pos_weight / 1,  L = (1/P) sum c_ij max(0, 1 - y_ij (b - d_ij)),
    a pair is active when 1 - y_ij (b - d_ij) > 0 (strictly).
"""
import math

import numpy as np
import torch


def init_w(dim, rank, seed):
    """MetricLearner's initial W: seeded N(0, 1/dim) from a CPU generator."""
    w = torch.randn((rank, dim), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    return (w * (1.0 / math.sqrt(dim))).numpy()


def pair_terms(z, labels, b, pos_weight):
    """Everything per pair, as full [n, n] fp64 / bool matrices (symmetric; `pair` is true for usable i != j)."""
    z = np.asarray(z, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    sq = (z * z).sum(1)
    d = np.maximum(0.0, sq[:, None] + sq[None, :] - 2.0 * (z @ z.T))
    ok = lab >= 0
    pair = ok[:, None] & ok[None, :] & ~np.eye(len(lab), dtype=bool)
    pos = lab[:, None] == lab[None, :]
    y = np.where(pos, 1.0, -1.0)
    c = np.where(pos, float(pos_weight), 1.0)
    arg = 1.0 - y * (float(b) - d)
    active = pair & (arg > 0.0)
    a = np.where(active, c * y, 0.0)
    return {"d": d, "pair": pair, "pos": pos, "y": y, "c": c, "arg": arg, "active": active, "a": a, "sq": sq}


def pair_grad_closed(z, labels, b, pos_weight):
    """(dz_unnorm [n, r] = 2 ((sum_j a_ij) z_i - sum_j a_ij z_j), stats [5]) as the pair kernel defines them:
    stats = {sum_{i<j} c h, P, active pairs, sum_{i<j} a, sum_{i<j} d}."""
    z = np.asarray(z, dtype=np.float64)
    t = pair_terms(z, labels, b, pos_weight)
    up = np.triu(t["pair"], 1)
    a = t["a"]
    dz = 2.0 * (a.sum(1)[:, None] * z - a @ z)
    h = np.where(t["active"], t["arg"], 0.0)
    stats = np.array([(t["c"] * h)[up].sum(), up.sum(), (t["active"] & up).sum(), a[up].sum(), t["d"][up].sum()],
                     dtype=np.float64)
    return dz, stats


def loss_and_grads_closed(x, w, b, labels, pos_weight):
    """(loss, dL/dW, dL/db) in numpy fp64 from the closed form; all zero when P = 0."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    dz, stats = pair_grad_closed(x @ w.T, labels, b, pos_weight)
    P = stats[1]
    if P == 0:
        return 0.0, np.zeros_like(w), 0.0
    return stats[0] / P, dz.T @ x / P, -stats[3] / P


def loss_and_grads_autograd(x, w, b, labels, pos_weight):
    """The same three values from torch fp64 autograd on the loss alone."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    w = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    bt = torch.tensor(float(b), dtype=torch.float64, requires_grad=True)
    lab = torch.as_tensor(np.asarray(labels).astype(np.int64))
    z = x @ w.T
    sq = (z * z).sum(1)
    d = torch.clamp(sq[:, None] + sq[None, :] - 2.0 * (z @ z.T), min=0.0)
    ok = lab >= 0
    up = torch.triu(ok[:, None] & ok[None, :], 1)
    pos = lab[:, None] == lab[None, :]
    y = torch.where(pos, 1.0, -1.0).to(torch.float64)
    c = torch.where(pos, float(pos_weight), 1.0).to(torch.float64)
    P = int(up.sum())
    if P == 0:
        return 0.0, np.zeros(tuple(w.shape)), 0.0
    loss = (c * torch.clamp(1.0 - y * (bt - d), min=0.0))[up].sum() / P
    loss.backward()
    return float(loss.detach()), w.grad.numpy(), float(bt.grad)


def calibrate(x, w, labels):
    """MetricLearner.calibrate: (W rescaled so that the mean pair distance is 2, b = 2)."""
    _, stats = pair_grad_closed(np.asarray(x, np.float64) @ np.asarray(w, np.float64).T, labels, 0.0, 1.0)
    mean = stats[4] / stats[1] if stats[1] > 0 else 0.0
    w = np.asarray(w, dtype=np.float64)
    return (w * math.sqrt(2.0 / mean) if mean > 0 else w), 2.0


def fit(x, labels, w0, steps, lr, mu=0.9, weight_decay=0.0, pos_weight=1.0):
    """MetricLearner.fit(batch=None) in fp64: calibrate, then `steps` full-batch momentum updates
    (m = mu m + (g + wd w), w -= lr m; no weight decay on b).  Returns (W, b, loss history)."""
    w, b = calibrate(x, w0, labels)
    mw, mb = np.zeros_like(w), 0.0
    hist = np.zeros(steps)
    for t in range(steps):
        hist[t], gw, gb = loss_and_grads_closed(x, w, b, labels, pos_weight)
        mw = mu * mw + (gw + weight_decay * w)
        mb = mu * mb + gb
        w = w - lr * mw
        b = b - lr * mb
    return w, b, hist


def self_map(rows, labels):
    """Leave-one-out retrieval mAP over squared L2 distances: ranking by (distance, id), AP over the full ranking,
    queries with a label < 0 or without a relevant row left out of the mean."""
    rows = np.asarray(rows, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    sq = (rows * rows).sum(1)
    d = np.maximum(0.0, sq[:, None] + sq[None, :] - 2.0 * (rows @ rows.T))
    ids = np.arange(len(lab))
    aps = []
    for q in range(len(lab)):
        if lab[q] < 0:
            continue
        order = np.lexsort((ids, d[q]))
        order = order[order != q]
        rel = lab[order] == lab[q]
        R = int(rel.sum())
        if R == 0:
            continue
        ranks = np.nonzero(rel)[0] + 1
        aps.append(np.sum(np.arange(1, R + 1) / ranks) / R)
    return float(np.mean(aps)) if aps else float("nan")
