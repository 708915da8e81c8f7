"""fp64 reference of the scorer's gradient (per-shape grouping, mean_score weights) for tests/test_gpu_scorer_train.py.

    r_b  = mean_p raw[b,p,:] . k_v + beta_v          s_b = |r_b| / (1 + |r_b|)
    M_g  = {v : gidx[n,v] = g}  (a CONSTANT: the binning has no gradient; a gidx outside [0, G) is in no group)
    w_g  = mean_{v in M_g} s_v  (0 for an empty group),  W = sum_g w_g
    D_g  = pool_{v in M_g} F_v,  S = sum_g w_g D_g / W   (0 when W = 0)

torch autograd in float64 on the CPU, from the STORED values of the inputs (a 16-bit input is rounded by the caller
first: q()).  Nothing of the product is imported: the arithmetic is written out here.  Every gradient comes back with
its absolute-term sum, the quantity the tests scale their tolerances by (a gradient here is a sum of terms of both signs).
"""
import torch

F64 = torch.float64


def q(t, tdt):
    """The values a tensor holds once stored as `tdt`, in float64."""
    return t.to(tdt).to(F64)


def members(gidx, G):
    """mask [N, G, V] (bool) of the group members and their counts [N, G]."""
    gi = torch.as_tensor(gidx).long()
    mask = gi[:, None, :] == torch.arange(G)[None, :, None]
    return mask, mask.sum(-1)


def pooled(F, mask, pool):
    """D [N, G, E]: max / mean over the members of every group; zeros for an empty group (it never enters S)."""
    N, G, V = mask.shape
    rows = []
    for n in range(N):
        for g in range(G):
            idx = torch.nonzero(mask[n, g]).reshape(-1)
            if idx.numel() == 0:
                rows.append(torch.zeros(F.shape[-1], dtype=F64))
            elif pool == "max":
                rows.append(torch.amax(F[n, idx], dim=0))
            else:
                rows.append(F[n, idx].mean(dim=0))
    return torch.stack(rows).reshape(N, G, -1)


def fuse(D, w, cnt):
    """S [N, E] = sum_g w_g D_g / W over the non-empty groups; 0 where W = 0."""
    we = torch.where(cnt > 0, w, torch.zeros_like(w))
    W = we.sum(-1)
    num = (we[:, :, None] * D).sum(1)
    safe = torch.where(W != 0, W, torch.ones_like(W))
    return torch.where((W != 0)[:, None], num / safe[:, None], torch.zeros_like(num)), W


def group_weight_grad(F, dS, gidx, weight, G, pool):
    """dL/dw [N, G] for L = sum S . dS, by autograd with respect to the weights, and its absolute-term sum
    A[n,g] = (1/W) sum_e |dS_e| (|D_{g,e}| + |S_e|).  F [N, V, E], dS [N, E], weight [N, G] (all float64)."""
    mask, cnt = members(gidx, G)
    w = weight.clone().to(F64).requires_grad_(True)
    D = pooled(F, mask, pool)
    S, W = fuse(D, w, cnt)
    (S * dS).sum().backward()
    dw = torch.where(cnt > 0, w.grad, torch.zeros_like(w.grad))
    Wd = W.detach()
    A = (dS.abs()[:, None, :] * (D.abs() + S.detach().abs()[:, None, :])).sum(-1)
    A = torch.where((Wd != 0)[:, None] & (cnt > 0), A / torch.where(Wd != 0, Wd, torch.ones_like(Wd)).abs()[:, None],
                    torch.zeros_like(A))
    return dw, A


def score_of(r):
    return r.abs() / (1.0 + r.abs())                  # sigmoid(log|r|)


def mean_score_weights(s, mask, cnt):
    """w [N, G] = mean of the member scores, 0 for an empty group."""
    tot = (mask.to(F64) * s[:, None, :]).sum(-1)
    return torch.where(cnt > 0, tot / cnt.clamp(min=1).to(F64), torch.zeros_like(tot))


def response_grad(r_img, gidx, dw, G, dw_abs=None):
    """dL/dr [N, V] for L = sum_{n,g} dw[n,g] w_g(s(r)), by autograd with respect to r, and its absolute-term sum (the
    same chain on dw_abs, default |dw|)."""
    mask, cnt = members(gidx, G)
    r = r_img.clone().to(F64).requires_grad_(True)
    (mean_score_weights(score_of(r), mask, cnt) * dw).sum().backward()
    r2 = r_img.clone().to(F64).abs().requires_grad_(True)          # |r|: every factor of the chain positive
    (mean_score_weights(score_of(r2), mask, cnt) * (dw.abs() if dw_abs is None else dw_abs)).sum().backward()
    return r.grad, torch.where(r_img != 0, r2.grad, torch.zeros_like(r2.grad))


def scorer_grad(raw, kernel, dr, dr_abs):
    """From dL/dr to the scorer and the raw tap, by autograd through r = mean_p raw . k + beta.
    raw [N, V, hw, cr], kernel [V, cr] (float64).  Returns dkernel [V, cr], dbias [V], the raw-tap term [N, V, hw, cr]
    and the absolute-term sums of dkernel and dbias."""
    k = kernel.clone().requires_grad_(True)
    b = torch.zeros(kernel.shape[0], dtype=F64, requires_grad=True)
    x = raw.clone().requires_grad_(True)
    r = (x.mean(2) * k[None]).sum(-1) + b[None]
    (r * dr).sum().backward()
    A_k = (dr_abs[:, :, None] * raw.abs().mean(2)).sum(0)
    A_b = dr_abs.sum(0)
    return k.grad, b.grad, x.grad, A_k, A_b


def head_chain(raw, F, dS, kernel, bias, gidx, G, pool):
    """The whole chain by ONE autograd pass: raw tap -> r -> s -> w -> S, L = sum S . dS, with the members fixed by gidx.
    raw [N, V, hw, cr], F [N, V, E], dS [N, E], kernel [V, cr], bias [V] (float64).
    Returns dict(dkernel, dbias, draw, dw, A_kernel, A_bias, r, s)."""
    mask, cnt = members(gidx, G)
    k = kernel.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    x = raw.clone().requires_grad_(True)
    r = (x.mean(2) * k[None]).sum(-1) + b[None]
    s = score_of(r)
    w = mean_score_weights(s, mask, cnt)
    w.retain_grad()
    D = pooled(F, mask, pool)
    S, W = fuse(D, w, cnt)
    (S * dS).sum().backward()
    dw = torch.where(cnt > 0, w.grad, torch.zeros_like(w.grad))
    # absolute-term sums, carried through the same chain: A_w -> |dr| bound -> sums over the shapes
    Wd = W.detach()
    A_w = (dS.abs()[:, None, :] * (D.abs() + S.detach().abs()[:, None, :])).sum(-1)
    A_w = torch.where((Wd != 0)[:, None] & (cnt > 0), A_w / torch.where(Wd != 0, Wd, torch.ones_like(Wd)).abs()[:, None],
                      torch.zeros_like(A_w))
    _, dr_abs = response_grad(r.detach(), gidx, dw, G, dw_abs=A_w)
    return dict(dkernel=k.grad, dbias=b.grad, draw=x.grad, dw=dw, A_w=A_w,
                A_kernel=(dr_abs[:, :, None] * raw.abs().mean(2)).sum(0), A_bias=dr_abs.sum(0),
                r=r.detach(), s=s.detach())
