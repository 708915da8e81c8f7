"""fp64 numpy restatement of the logit attribution of csrc/explain.hip (include/gvcnn_hip.h: gv_explain_views).

F is taken AS STORED (already cast to the storage type and back).  Every output comes back as a triple
(value, n, T): n the number of terms summed into it, T the sum of their absolute values, so a test can bound the fp32
result by (n + const) * 2^-24 * T without looking at the code under test.
"""
import numpy as np


def _per_shape(scheme, weight, n):
    scheme, weight = np.asarray(scheme), np.asarray(weight, dtype=np.float64)
    return (scheme[n], weight[n]) if scheme.ndim == 3 else (scheme, weight)


def forward_logits(F, scheme, weight, K, b, pool="max", fill=1.0):
    """The head itself in fp64: view pooling, group fusion, global average pool, Dense.  F [N,V,hw,C] -> [N, classes]."""
    F, K, b = np.asarray(F, np.float64), np.asarray(K, np.float64), np.asarray(b, np.float64)
    N, V, hw, C = F.shape
    out = np.zeros((N, K.shape[1]))
    for n in range(N):
        sch, w = _per_shape(scheme, weight, n)
        W = w.sum()
        S = np.zeros((hw, C))
        if W != 0:
            for g in range(sch.shape[0]):
                m = sch[g] != 0
                if not m.any():
                    D = np.full((hw, C), float(fill))
                else:
                    D = F[n][m].max(0) if pool == "max" else F[n][m].mean(0)
                S += w[g] * D
            S /= W
        out[n] = S.mean(0) @ K + b
    return out


def gradient(F, scheme, weight, K, targets, pool="max"):
    """(dlogit_k/dF, the same with every term's absolute value, groups per view [N,V]) — grouping held constant, a
    tied maximum split equally."""
    F, K = np.asarray(F, np.float64), np.asarray(K, np.float64)
    N, V, hw, C = F.shape
    grad, agrad = np.zeros_like(F), np.zeros_like(F)
    ngroups = np.zeros((N, V), dtype=np.int64)
    for n in range(N):
        sch, w = _per_shape(scheme, weight, n)
        W = w.sum()
        if W == 0:
            continue
        for g in range(sch.shape[0]):
            m = sch[g] != 0
            if not m.any():
                continue
            Fg = F[n][m]
            if pool == "max":
                tie = Fg == Fg.max(0, keepdims=True)
                share = tie / tie.sum(0, keepdims=True)
            else:
                share = np.full(Fg.shape, 1.0 / m.sum())
            grad[n][m] += (w[g] / W) * share
            agrad[n][m] += abs(w[g] / W) * share
            ngroups[n][m] += 1
        kc = K[:, int(targets[n])] / hw
        grad[n] *= kc
        agrad[n] *= np.abs(kc)
    return grad, agrad, ngroups


def explain(F, scheme, weight, K, b, targets, pool="max", fill=1.0, kind="exact"):
    """dict: maps [N,V,hw], view_contrib [N,V], baseline [N] (and alpha [N,V,C] for gradcam), each (value, n, T)."""
    F, K, b = np.asarray(F, np.float64), np.asarray(K, np.float64), np.asarray(b, np.float64)
    N, V, hw, C = F.shape
    grad, agrad, ng = gradient(F, scheme, weight, K, targets, pool)
    term, aterm = F * grad, np.abs(F) * agrad
    exact = (term.sum(3), np.broadcast_to((C * ng)[:, :, None], (N, V, hw)).copy(), aterm.sum(3))
    out = {"view_contrib": (term.sum((2, 3)), hw * C * ng, aterm.sum((2, 3)))}
    base, bn, bT = np.zeros(N), np.ones(N, dtype=np.int64), np.zeros(N)
    for n in range(N):
        k = int(targets[n])
        sch, w = _per_shape(scheme, weight, n)
        W = w.sum()
        base[n], bT[n] = b[k], abs(b[k])
        if W == 0:
            continue
        for g in range(sch.shape[0]):
            if not (sch[g] != 0).any():
                base[n] += (w[g] / W) * fill * K[:, k].sum()
                bT[n] += abs(w[g] / W) * abs(fill) * np.abs(K[:, k]).sum()
                bn[n] += C
    out["baseline"] = (base, bn, bT)
    if kind == "exact":
        out["maps"] = exact
        return out
    alpha, aalpha = grad.sum(2) / hw, agrad.sum(2) / hw                      # [N,V,C]
    out["alpha"] = (alpha, np.broadcast_to((hw * ng)[:, :, None], (N, V, C)).copy(), aalpha)
    cam = (alpha[:, :, None, :] * F).sum(3)
    out["maps"] = (np.maximum(cam, 0.0), np.broadcast_to((C * hw * ng)[:, :, None], (N, V, hw)).copy(),
                   (aalpha[:, :, None, :] * np.abs(F)).sum(3))
    return out
