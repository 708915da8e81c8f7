"""Reference of the grouping head (helper, not collected): the operations between the backbone's last tap and the logits
(csrc/grouping.hip and csrc/pool.hip: one kernel template per op for every storage type), restated twice from the STORED
values.

fp64 (plain torch, on the device of the inputs; a bf16 / fp16 / fp32 tensor is widened exactly):
    r_img[b] = mean_p(raw[b,p,:] . k[v(b)]) + bias[v(b)]        v(b) = b % V (shape-major) or b // N (view-major)
    score    = |r| / (1 + |r|),  r the batch mean over n         the closed form of sigmoid(log|r|)
    D_g      = max / mean over the views of group g, `fill` for an empty group
    S        = sum_g w_g D_g / sum_g w_g, 0 where sum w == 0
    scale-shift-ReLU, global average pool, dense, argmax (first maximum) / confusion / correct
Every reduction also returns sum |terms|: the error bounds of the sweep are stated against it.

Ordered fp32 (numpy, CPU), where the kernel fixes the order of its operations:
    view pool + fuse: max is exact; mean adds the group's views in ascending view index and divides once by the count;
    the fusion adds fl(w * d) in ascending g and divides once by wsum, itself the ascending fp32 sum of the weights; for
    16-bit storage one round-to-nearest-even into the storage type follows (D and S each from the unrounded fp32 value).
    group_assign / group_assign_per_shape: bin = int(float32(s) * float32(num_bins)); weights 1 + count, or the fp32 sum
    of the group's scores in view order followed by one division.
numpy's float32 +, *, / are single IEEE operations, so the restatement is the kernel's arithmetic element for element.
"""
import numpy as np
import torch

from oracle import grouping as OG

F32 = np.float32
SHAPE_MAJOR, VIEW_MAJOR = 0, 1


def view_of_image(nb, V, order):
    """v(b) for b in range(nb): image b of a [N, V] (shape-major) or [V, N] (view-major) batch."""
    b = np.arange(nb)
    return b % V if order == SHAPE_MAJOR else b // (nb // V)


# ---- fp64 ---------------------------------------------------------------------------------------------------------------
def score_partial(raw, kernel, bias, V, order):
    """raw [nb, hw, cr], kernel [V, cr], bias [V] -> (r_img [nb], sum |terms| [nb]) in float64; sum |terms| is
    sum_{p,c} |raw * k| before the division by hw."""
    nb, hw, _ = raw.shape
    v = torch.as_tensor(view_of_image(nb, V, order), device=raw.device)
    terms = raw.double() * kernel.double()[v][:, None, :]
    return terms.sum((1, 2)) / hw + bias.double()[v], terms.abs().sum((1, 2))


def score_closed(r):
    """|r| / (1 + |r|) in float64: 0 for r = +-0, 1 for r = +-inf, NaN for NaN."""
    a = torch.as_tensor(r).double().abs()
    return torch.where(torch.isinf(a), torch.ones_like(a), a / (1.0 + a))


def view_score(r_img, N, V, order):
    """r_img [N*V] -> (score [V], batch mean r [V], mean_n |r_img| [V]) in float64."""
    r = r_img.double().reshape(N, V) if order == SHAPE_MAJOR else r_img.double().reshape(V, N).t()
    m = r.mean(0)
    return score_closed(m), m, r.abs().mean(0)


def view_score_per_shape(r_img):
    return score_closed(r_img)


def _scheme3(scheme, N):
    s = np.asarray(scheme)
    return np.broadcast_to(s, (N,) + s.shape[-2:]) if s.ndim == 2 else s


def pool_fuse(F, scheme, weight, mode, fill):
    """F [N, V, E] (any strides), scheme [G, V] or [N, G, V], weight [G] or [N, G] -> (D [G, N, E], S [N, E]) in float64.
    Differentiable in F (the backward kernel's reference is autograd through this)."""
    N, V, E = F.shape
    sch = torch.as_tensor(np.array(_scheme3(scheme, N)), device=F.device) != 0          # [N, G, V]
    w = torch.as_tensor(np.asarray(weight), device=F.device).double()
    w = w.expand(N, -1) if w.dim() == 1 else w
    Fd = F.double()
    shared = np.asarray(scheme).ndim == 2                                # one scheme for the batch: all shapes at once
    D = []
    for g in range(sch.shape[1]):
        rows = []
        for n0, n1 in ([(0, N)] if shared else [(n, n + 1) for n in range(N)]):
            idx = torch.nonzero(sch[n0, g]).reshape(-1)
            if idx.numel() == 0:
                rows.append(torch.full((n1 - n0, E), float(fill), dtype=torch.float64, device=F.device))
            else:
                sel = Fd[n0:n1, idx]
                rows.append(torch.amax(sel, 1) if mode == "max" else sel.mean(1))
        D.append(torch.cat(rows))
    D = torch.stack(D)                                                   # [G, N, E]
    wsum = w.sum(1)
    num = (w.t()[:, :, None] * D).sum(0)
    safe = torch.where(wsum != 0, wsum, torch.ones_like(wsum))
    S = torch.where((wsum != 0)[:, None], num / safe[:, None], torch.zeros_like(num))
    return D, S


def scale_shift_act(x, scale, shift, relu):
    """x [npix, c] -> (y, |x * scale| + |shift|) in float64."""
    t = x.double() * scale.double()
    y = t + shift.double()
    return (y.clamp_min(0.0) if relu else y), t.abs() + shift.double().abs()


def global_avg_pool(x):
    """x [nb, hw, c] -> (mean over hw [nb, c], sum_p |x| [nb, c]) in float64."""
    xd = x.double()
    return xd.mean(1), xd.abs().sum(1)


def dense(x, kernel, bias):
    """x [n, f] @ kernel [f, c] + bias [c] -> (y, sum_i |x_i k_ic| + |bias_c|) in float64."""
    xd, kd, bd = x.double(), kernel.double(), bias.double()
    return xd @ kd + bd, xd.abs() @ kd.abs() + bd.abs()


def eval_metrics(logits, labels, confusion0=None, correct0=0):
    """numpy: argmax (first maximum) per row; confusion[label, prediction] and the correct count ADDED to their starting
    values; labels outside [0, c) are counted nowhere."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    n, c = logits.shape
    pred = logits.argmax(axis=1)
    conf = np.zeros((c, c), np.int64) if confusion0 is None else np.array(confusion0, dtype=np.int64)
    ok = (labels >= 0) & (labels < c)
    np.add.at(conf, (labels[ok], pred[ok]), 1)
    return pred, conf, int(correct0) + int((pred[ok] == labels[ok]).sum())


# ---- ordered fp32 -------------------------------------------------------------------------------------------------------
def pool_fuse_f32(F, scheme, weight, mode, fill):
    """F [N, V, E] float32 ndarray -> (D [G, N, E], S [N, E]) float32, the operations in the kernel's order."""
    F = np.asarray(F, dtype=F32)
    N, V, E = F.shape
    sch = _scheme3(scheme, N)
    G = sch.shape[1]
    w = np.asarray(weight, dtype=F32)
    w = np.broadcast_to(w, (N, G)) if w.ndim == 1 else w
    D = np.empty((G, N, E), F32)
    S = np.zeros((N, E), F32)
    shared = np.asarray(scheme).ndim == 2
    for n0, n1 in ([(0, N)] if shared else [(n, n + 1) for n in range(N)]):
        acc = np.zeros((n1 - n0, E), F32)
        wsum = F32(0)
        for g in range(G):
            idx = np.nonzero(sch[n0, g])[0]
            if idx.size == 0:
                d = np.full((n1 - n0, E), fill, F32)
            else:
                d = F[n0:n1, idx[0]].copy()
                for v in idx[1:]:
                    d = np.maximum(d, F[n0:n1, v]) if mode == "max" else d + F[n0:n1, v]
                if mode == "mean":
                    d = d / F32(idx.size)
            D[g, n0:n1] = d
            acc = acc + w[n0, g] * d
            wsum = F32(wsum + w[n0, g])
        if wsum != 0:
            S[n0:n1] = acc / wsum
    assert D.dtype == F32 and S.dtype == F32
    return D, S


def group_assign_f32(scores, G, num_bins, weight_mode="count"):
    """scores [V] -> (gidx [V] int32, scheme [G, V] int32, weight [G] float32, status).  The kernels' contract for the
    status cases: NaN -> gidx -1, status |= 2; a bin outside [0, G) -> status |= 1 and the view is in no group."""
    s = np.asarray(scores, dtype=F32)
    V = s.shape[0]
    gidx, status = np.empty(V, np.int32), 0
    for v in range(V):
        if s[v] != s[v]:
            gidx[v], status = -1, status | 2
            continue
        gidx[v] = int(F32(s[v]) * F32(num_bins))
        if gidx[v] >= G or gidx[v] < 0:
            status |= 1
    scheme = (gidx[None, :] == np.arange(G)[:, None]).astype(np.int32)
    if weight_mode == "count":
        weight = (1 + scheme.sum(1)).astype(F32)
    else:
        weight = OG.group_weight_mean_score(scheme, s)
    return gidx, scheme, weight, status


def group_assign_per_shape_f32(scores, G, num_bins, weight_mode):
    """scores [N, V] -> (gidx [N, V], scheme [N, G, V], weight [N, G], status or-ed over the shapes)."""
    outs = [group_assign_f32(row, G, num_bins, weight_mode) for row in np.asarray(scores, dtype=F32)]
    status = 0
    for o in outs:
        status |= o[3]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]), status
