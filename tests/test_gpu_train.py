"""Training step: every backward kernel against torch autograd through the CPU oracle's
forward ops, then the whole step (train-mode forward, loss, all gradients, Momentum) against
oracle/train.py.  fp32; tolerance relative to each tensor's scale (BatchNorm on batch statistics
amplifies rounding noise by 1/sigma, so gradients are held to 2e-3 of their scale)."""
import ctypes as C

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib                       # noqa: E402
from gvcnn_tf_amd.training import TrainGVCNN        # noqa: E402
from oracle import backbone as OB                   # noqa: E402
from oracle import train as OT                      # noqa: E402

DEV = "cuda:0"


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def close(a, d, tol=2e-3):
    a, d = np.asarray(a, dtype=np.float64), np.asarray(d, dtype=np.float64)
    scale = max(float(np.abs(d).max()), 1e-30)
    err = float(np.abs(a - d).max())
    assert err <= tol * scale, "max|diff| %.3e vs scale %.3e (%.2e rel)" % (err, scale, err / scale)


def test_bn_train_forward_and_backward_grouped():
    g = torch.Generator().manual_seed(0)
    N, V, h, w, c = 3, 4, 5, 6, 32
    z = torch.randn(N * V, h, w, c, generator=g) * 2 + 0.5
    beta, gamma = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    dy = torch.randn(N * V, h, w, c, generator=g)
    groups = [b % V for b in range(N * V)]
    for gm in (None, gamma):
        zz = z.clone().requires_grad_(True)
        be = beta.clone().requires_grad_(True)
        ga = gm.clone().requires_grad_(True) if gm is not None else None
        y_ref, mean_ref, var_ref = OB.batch_norm_train_grouped(zz, be, ga, 1e-3, groups)
        y_ref = torch.relu(y_ref)
        y_ref.backward(dy)
        zd = z.to(DEV)
        counts = torch.full((V,), N * h * w, dtype=torch.int32, device=DEV)
        accum = torch.zeros(2 * V * c, dtype=torch.float64, device=DEV)
        stt = {k: torch.empty(V, c, device=DEV) for k in ("mean", "var", "inv", "scale", "shift")}
        bd, gd = beta.to(DEV), (gm.to(DEV) if gm is not None else None)
        _lib.check(lib().gv_bn_stats_grouped(zd.data_ptr(), N * V, h * w, c, c, V, counts.data_ptr(),
                                             gd.data_ptr() if gd is not None else None, bd.data_ptr(), 1e-3,
                                             accum.data_ptr(), stt["mean"].data_ptr(), stt["var"].data_ptr(),
                                             stt["inv"].data_ptr(), stt["scale"].data_ptr(), stt["shift"].data_ptr(),
                                             st()), "stats")
        yd = torch.empty_like(zd)
        _lib.check(lib().gv_scale_shift_act_grouped(zd.data_ptr(), N * V, h * w, c, c, stt["scale"].data_ptr(),
                                                    stt["shift"].data_ptr(), V, 1, yd.data_ptr(), c, st()), "apply")
        close(stt["mean"].cpu(), mean_ref.detach(), 1e-5)
        close(stt["var"].cpu(), var_ref.detach(), 1e-5)
        close(yd.cpu(), y_ref.detach(), 1e-5)
        dyd = dy.to(DEV)
        dz = torch.zeros_like(zd)
        dbeta = torch.zeros(c, device=DEV)
        dgamma = torch.zeros(c, device=DEV)
        _lib.check(lib().gv_bn_relu_bwd_grouped(dyd.data_ptr(), c, yd.data_ptr(), c, zd.data_ptr(), c,
                                                stt["mean"].data_ptr(), stt["inv"].data_ptr(),
                                                gd.data_ptr() if gd is not None else None, counts.data_ptr(), N * V,
                                                h * w, c, V, accum.data_ptr(), dz.data_ptr(), c, dbeta.data_ptr(),
                                                dgamma.data_ptr() if gd is not None else None, st()), "bn_bwd")
        close(dz.cpu(), zz.grad, 1e-4)
        close(dbeta.cpu(), be.grad, 1e-5)
        if gm is not None:
            close(dgamma.cpu(), ga.grad, 1e-4)


@pytest.mark.parametrize("k,stride,padding,mode", [(3, 2, "VALID", "max"), (3, 2, "SAME", "max"),
                                                    (3, 1, "SAME", "avg"), (1, 2, "VALID", "max")])
def test_pool_backward(k, stride, padding, mode):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 8, 16, generator=g).requires_grad_(True)
    y = OB.max_pool2d(x, k, stride, padding) if mode == "max" else OB.avg_pool2d_same3(x)
    dy = torch.randn(*y.shape, generator=g)
    y.backward(dy)
    pt = OB.same_pads(9, k, stride)[0] if padding == "SAME" else 0
    pl = OB.same_pads(8, k, stride)[0] if padding == "SAME" else 0
    d = _lib.PoolDesc(2, 9, 8, 16, 16, k, k, stride, pt, pl, y.shape[1], y.shape[2], 16,
                      _lib.GV_POOL_MAX if mode == "max" else _lib.GV_POOL_AVG, _lib.GV_F32)
    xd, dyd = x.detach().to(DEV), dy.to(DEV)
    dx = torch.zeros_like(xd)
    _lib.check(lib().gv_pool2d_bwd(C.byref(d), xd.data_ptr(), dyd.data_ptr(), 16, dx.data_ptr(), 16, st()), "pool_bwd")
    close(dx.cpu(), x.grad, 1e-5)
    # store form over garbage: same gradient
    d.mode |= _lib.GV_POOL_BWD_STORE
    dxs = torch.full_like(xd, float("nan"))
    _lib.check(lib().gv_pool2d_bwd(C.byref(d), xd.data_ptr(), dyd.data_ptr(), 16, dxs.data_ptr(), 16, st()), "pool_bwd")
    assert torch.equal(dxs, dx)


@pytest.mark.parametrize("k,stride,padding,cin,cout", [((3, 3), 1, "SAME", 32, 48), ((3, 3), 2, "VALID", 32, 64),
                                                       ((1, 7), 1, "SAME", 48, 32), ((5, 5), 1, "SAME", 48, 64),
                                                       ((3, 3), 1, "VALID", 80, 96), ((1, 1), 1, "SAME", 96, 32),
                                                       ((3, 3), 2, (1, 1, 1, 1), 64, 64), ((1, 1), 2, "VALID", 64, 128),
                                                       ((3, 3), 2, "VALID", 3, 32)])
def test_conv_dgrad_and_wgrad_vs_autograd(k, stride, padding, cin, cout):
    g = torch.Generator().manual_seed(hash((k, stride, cin)) % 997)
    nb, ih, iw = 3, 12, 11
    x = torch.randn(nb, ih, iw, cin, generator=g).requires_grad_(True)
    w = (torch.randn(k[0], k[1], cin, cout, generator=g) * 0.1).requires_grad_(True)
    z = OB.conv2d(x, w, stride, padding)
    dz = torch.randn(*z.shape, generator=g)
    z.backward(dz)
    oh, ow = z.shape[1:3]
    if isinstance(padding, str):
        pt = OB.same_pads(ih, k[0], stride)[0] if padding == "SAME" else 0
        pl = OB.same_pads(iw, k[1], stride)[0] if padding == "SAME" else 0
    else:
        pt, pl = padding[0], padding[2]
    math = _lib.GV_MATH_BF16X3
    xd, dzd = x.detach().to(DEV), dz.to(DEV)
    # filter gradient
    dw = torch.zeros(k[0], k[1], cin, cout, device=DEV)
    d = _lib.ConvDesc(nb, ih, iw, cin, cin, k[0], k[1], stride, pt, pl, oh, ow, cout, cout, 0, 0, 0, _lib.GV_F32,
                      0, 0, math, 0)
    _lib.check(lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), cout, dw.data_ptr(), st()), "wgrad")
    close(dw.cpu(), w.grad, 2e-5)
    if cin % 16:
        return                                            # the stem's input image needs no data gradient
    # data gradient = forward kernel on dilated dZ with the flipped/transposed filter, accumulating
    wt = torch.flip(w.detach(), (0, 1)).permute(0, 1, 3, 2).contiguous().to(DEV)
    n = lib().gv_packed_filter_bytes(k[0], k[1], cout, cin, _lib.GV_F32, math) // 4
    wp = torch.empty(n, device=DEV)
    _lib.check(lib().gv_pack_filter_hwio(wt.data_ptr(), k[0], k[1], cout, cin, wp.data_ptr(), _lib.GV_F32, math, st()),
               "pack")
    dx = torch.full((nb, ih, iw, cin), 0.25, device=DEV)          # pre-existing gradient: must be accumulated into
    ones, zeros = torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV)
    dd = _lib.ConvDesc(nb, oh, ow, cout, cout, k[0], k[1], 1, k[0] - 1 - pt, k[1] - 1 - pl, ih, iw, cin, cin, cin, 0,
                       0, _lib.GV_F32, 0, 0, math, stride if stride > 1 else 0)
    _lib.check(lib().gv_conv2d_fwd(C.byref(dd), dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(),
                                   dx.data_ptr(), dx.data_ptr(), None, None, None, st()), "dgrad")
    close(dx.cpu() - 0.25, x.grad, 2e-5)


def test_view_pool_fuse_backward_ties_and_empty_groups():
    g = torch.Generator().manual_seed(3)
    V, N, G = 6, 2, 5
    F = torch.randint(-2, 3, (N, V, 3, 3, 8), generator=g).float()         # small integers => many ties
    scheme = np.zeros((G, V), dtype=np.int32)
    scheme[0, [0, 3]] = 1
    scheme[2, [1, 2, 4]] = 1
    scheme[4, 5] = 1
    weight = np.array([3, 1, 4, 1, 2], dtype=np.float32)
    for mode in ("max", "mean"):
        Fr = F.clone().requires_grad_(True)
        acc = 0
        for gi in range(G):
            idx = np.nonzero(scheme[gi])[0]
            if idx.size:
                sel = Fr[:, torch.as_tensor(idx)]
                d = torch.amax(sel, dim=1) if mode == "max" else sel.mean(dim=1)
            else:
                d = torch.ones_like(Fr[:, 0])
            acc = acc + float(weight[gi]) * d
        S = acc / float(weight.sum())
        dS = torch.randn(*S.shape, generator=g)
        S.backward(dS)
        Fd, dSd = F.to(DEV).contiguous(), dS.to(DEV).contiguous()
        dF = torch.zeros_like(Fd)
        E = 3 * 3 * 8
        sch = torch.from_numpy(scheme).to(DEV)
        wd = torch.from_numpy(weight).to(DEV)
        _lib.check(lib().gv_view_pool_fuse_bwd(Fd.data_ptr(), dSd.data_ptr(), V, N, E, E, V * E, sch.data_ptr(), G,
                                               wd.data_ptr(), 0 if mode == "max" else 1, dF.data_ptr(), st()), "vp_bwd")
        close(dF.cpu(), Fr.grad, 1e-5)


def test_loss_dense_gap_and_momentum():
    g = torch.Generator().manual_seed(4)
    n, f, c = 5, 64, 7
    gap = torch.randn(n, f, generator=g).requires_grad_(True)
    Wk = (torch.randn(f, c, generator=g) * 0.1).requires_grad_(True)
    b = torch.randn(c, generator=g).requires_grad_(True)
    labels = torch.randint(0, c, (n,), generator=g)
    logits = gap @ Wk + b
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    ld = logits.detach().to(DEV)
    lossd, dl = torch.zeros(1, device=DEV), torch.empty(n, c, device=DEV)
    lab = labels.to(DEV)
    _lib.check(lib().gv_softmax_ce(ld.data_ptr(), lab.data_ptr(), n, c, lossd.data_ptr(), dl.data_ptr(), st()), "ce")
    close(lossd.cpu(), [float(loss)], 1e-5)
    gd, Wd = gap.detach().to(DEV), Wk.detach().to(DEV)
    dgap, dW, db = torch.empty(n, f, device=DEV), torch.zeros(f, c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib().gv_dense_bwd(gd.data_ptr(), dl.data_ptr(), Wd.data_ptr(), n, f, c, dgap.data_ptr(), dW.data_ptr(),
                                  db.data_ptr(), st()), "dense_bwd")
    close(dgap.cpu(), gap.grad, 1e-5)
    close(dW.cpu(), Wk.grad, 1e-5)
    close(db.cpu(), b.grad, 1e-5)
    dx = torch.zeros(n, 6, f, device=DEV)
    _lib.check(lib().gv_global_avg_pool_bwd(dgap.data_ptr(), n, 6, f, dx.data_ptr(), f, st()), "gap_bwd")
    close(dx.cpu(), (gap.grad / 6)[:, None, :].expand(n, 6, f), 1e-5)
    # Momentum (train.py:171) with the slim L2 term
    w0, g0, m0 = torch.randn(100, generator=g), torch.randn(100, generator=g), torch.randn(100, generator=g)
    wd_, gd_, md_ = w0.to(DEV), g0.to(DEV), m0.to(DEV)
    _lib.check(lib().gv_sgd_momentum(wd_.data_ptr(), gd_.data_ptr(), md_.data_ptr(), 100, 0.01, 0.9, 1e-4, st()), "sgd")
    m1 = 0.9 * m0 + (g0 + 1e-4 * w0)
    close(md_.cpu(), m1, 1e-6)
    close(wd_.cpu(), w0 - 0.01 * m1, 1e-6)


@pytest.mark.parametrize("n,c", [(300, 40), (1, 3)])
def test_softmax_ce_past_one_pass_of_the_block(n, c):
    """gv_softmax_ce with more rows than the block has threads (each thread takes rows i, i + 256, ...) and with one row: a
    logit of 80 makes the max-subtraction matter (exp(80) overflows fp32).  Against torch's cross_entropy in float64."""
    g = torch.Generator().manual_seed(40 + n)
    logits = torch.randn(n, c, generator=g) * 3
    logits[n // 2, 1] = 80.0
    labels = torch.randint(0, c, (n,), generator=g)
    labels[n // 2] = 2                                   # (not the large logit: the row's loss is ~80)
    l64 = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(l64, labels)
    loss.backward()
    lossd, dl = torch.full((1,), float("nan"), device=DEV), torch.full((n, c), float("nan"), device=DEV)
    ld, lab = logits.to(DEV), labels.to(DEV)
    _lib.check(lib().gv_softmax_ce(ld.data_ptr(), lab.data_ptr(), n, c, lossd.data_ptr(), dl.data_ptr(), st()), "ce")
    close(lossd.cpu(), [float(loss)], 1e-5)
    close(dl.cpu(), l64.grad, 1e-5)


@pytest.mark.parametrize("n,f,c", [(40, 24, 5), (3, 2048, 40)])
def test_dense_backward_accumulates_and_stores(n, f, c):
    """gv_dense_bwd with n*f > f*c and with f*c > n*f (one flat grid covers the three index ranges), more than one block:
    dW and db start non-zero (the contract is +=), dx starts as NaN (it is stored).  Against float64."""
    g = torch.Generator().manual_seed(n + f)
    x, dy = torch.randn(n, f, generator=g), torch.randn(n, c, generator=g)
    Wk = torch.randn(f, c, generator=g) * 0.1
    dW0, db0 = torch.randn(f, c, generator=g), torch.randn(c, generator=g)
    dx, dW, db = torch.full((n, f), float("nan"), device=DEV), dW0.to(DEV), db0.to(DEV)
    xd, dyd, Wd = x.to(DEV), dy.to(DEV), Wk.to(DEV)
    _lib.check(lib().gv_dense_bwd(xd.data_ptr(), dyd.data_ptr(), Wd.data_ptr(), n, f, c, dx.data_ptr(), dW.data_ptr(),
                                  db.data_ptr(), st()), "dense_bwd")
    close(dx.cpu(), dy.double() @ Wk.double().T, 1e-5)
    close(dW.cpu().double() - dW0.double(), x.double().T @ dy.double(), 1e-5)
    close(db.cpu().double() - db0.double(), dy.double().sum(0), 1e-5)


def test_global_avg_pool_backward_into_a_slice_and_ragged_momentum():
    """gv_global_avg_pool_bwd adds dgap / hw into a channel slice of a wider gradient buffer that already holds values (the
    other channels keep their sentinel); gv_sgd_momentum at n = 1000 (a ragged last block).  Against float64."""
    g = torch.Generator().manual_seed(6)
    n, hw, c, ld = 5, 9, 70, 96
    dgap = torch.randn(n, c, generator=g)
    dx0 = torch.randn(n, hw, c, generator=g)
    dx = torch.full((n, hw, ld), -7.0, device=DEV)
    dx[..., :c] = dx0.to(DEV)
    dgd = dgap.to(DEV)
    _lib.check(lib().gv_global_avg_pool_bwd(dgd.data_ptr(), n, hw, c, dx.data_ptr(), ld, st()), "gap_bwd")
    close(dx[..., :c].cpu().double() - dx0.double(), (dgap.double() / hw)[:, None, :].expand(n, hw, c), 1e-5)
    assert bool((dx[..., c:] == -7.0).all())
    nw = 1000
    w0, g0, m0 = torch.randn(nw, generator=g), torch.randn(nw, generator=g), torch.randn(nw, generator=g)
    wd_, gd_, md_ = w0.to(DEV), g0.to(DEV), m0.to(DEV)
    _lib.check(lib().gv_sgd_momentum(wd_.data_ptr(), gd_.data_ptr(), md_.data_ptr(), nw, 0.01, 0.9, 1e-4, st()), "sgd")
    m1 = 0.9 * m0.double() + (g0.double() + 1e-4 * w0.double())
    close(md_.cpu(), m1, 1e-6)
    close(wd_.cpu(), w0.double() - 0.01 * m1, 1e-6)
    assert torch.equal(gd_.cpu(), g0)


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_training_step_vs_oracle(backbone, size, N, V):
    """Whole step against torch autograd through the oracle (CPU).  Train-mode BN over a handful of
    samples per (view, channel) is ill-conditioned: the two fp32 forwards differ by ~3e-4 of the
    activation scale, which flips a few ReLU masks near zero, and each flip moves a channel's gradient by
    O(1/#samples).  So the oracle comparison is norm-wise (per tensor, L2) with a 6 % bound — the exactness
    of every backward kernel is established one by one above (1e-5), and the directional-derivative test
    below checks the assembled gradient against the engine's own loss."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    shapes = eng.plan.param_shapes()
    assert shapes == OB.trace_param_shapes(backbone)
    P = gv.params.init_backbone_params(shapes, seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    x = torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5
    labels = torch.tensor([1, 4, 2, 0][:N])
    ref = OT.loss_and_grads(x, labels.numpy(), P, Hd, G, backbone)
    scores, S, logits, loss = eng.forward(x.to(DEV), labels)
    assert eng.scheme.cpu().numpy().tolist() == ref["scheme"].tolist()
    close(S.cpu(), ref["shape_descriptor"], 2e-3)
    close(logits.cpu(), ref["logits"], 2e-3)
    assert abs(float(loss) - ref["loss"]) <= 2e-3 * max(1.0, abs(ref["loss"]))
    grads = eng.backward()
    torch.cuda.synchronize()
    assert set(ref["grads"]) <= set(grads)            # scorer layers / unused variables get none
    errs = []
    for name, gref in ref["grads"].items():
        a, d = grads[name].cpu().numpy().astype(np.float64), gref.numpy().astype(np.float64)
        errs.append((np.linalg.norm(a - d), np.linalg.norm(d), name))
    big = max(n for _, n, _ in errs)
    for e, n, name in errs:
        if n > 1e-3 * big:
            assert e <= 6e-2 * n, (name, e / n)
        else:                                          # numerically-zero gradients (a bias in front of a BN)
            assert e <= 1e-4 * big, (name, e, big)
    # one Momentum step moves the loss down on the same batch
    l0 = float(loss)
    eng.apply_momentum(lr=1e-5, mu=0.9, weight_decay=1e-4)
    _, _, _, loss1 = eng.forward(x.to(DEV), labels, g_scheme=ref["scheme"], g_weight=ref["weight"])
    assert float(loss1) < l0


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_assembled_step_with_frozen_statistics_vs_oracle(backbone, size, N, V, math="bf16x3"):
    """The WHOLE assembled step — forward, loss, every backward kernel chained through ~50 layers, fused siblings, lazy
    first-writer stores — against torch autograd through the oracle evaluated in fp64, with BatchNorm normalising by the
    moving statistics (TrainGVCNN(frozen_bn=True) / oracle loss_and_grads(frozen_bn=True)).  Without the
    batch-statistics feedback that amplifies rounding (see the fp64-arbiter test) the step is well-conditioned up to ONE
    discrete effect: an activation within the forward's rounding distance of zero gets a different ReLU mask, and on
    these small test tensors a single flipped element is 1-3e-3 of a gradient's norm.  Measured per (view, layer): the
    activation gradients agree with fp64 to 4e-6 from the loss down to the first such element of that view and to 1.5-5e-3
    below it (ResNet: view 0 down to block2/unit_2, view 1 down to block3/unit_5); the fp32 oracle, whose forward is ~10x
    closer to fp64, has fewer flips (1e-6 / 3e-3 worst on ResNet / Inception).  Asserted: forward quantities to 1e-4, the
    classifier and the last block to 1e-4 (above every flip: the chain of kernels itself is exact to rounding), every
    variable's gradient to 5e-3 norm-wise.  Train-mode BatchNorm itself is held kernel by kernel at 1e-5 above."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    del eng
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, math=math,
                     frozen_bn=True)
    x = torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5
    labels = torch.tensor([1, 4, 2, 0][:N])
    r32 = OT.loss_and_grads(x, labels.numpy(), P, Hd, G, backbone, frozen_bn=True)
    r64 = OT.loss_and_grads(x.double(), labels.numpy(), {k: torch.as_tensor(v).double() for k, v in P.items()},
                            {k: torch.as_tensor(v).double() for k, v in Hd.items()}, G, backbone, frozen_bn=True)
    scores, S, logits, loss = eng.forward(x.to(DEV), labels)
    assert eng.scheme.cpu().numpy().tolist() == r64["scheme"].tolist()
    close(S.cpu(), r64["shape_descriptor"], 1e-4)
    close(logits.cpu(), r64["logits"], 1e-4)
    assert abs(float(loss) - r64["loss"]) <= 1e-4 * max(1.0, abs(r64["loss"]))
    grads = eng.backward()
    torch.cuda.synchronize()
    assert set(r64["grads"]) <= set(grads)
    big = max(float(g.norm()) for g in r64["grads"].values())
    rows = []
    for name, g64 in r64["grads"].items():
        g64 = g64.numpy()
        n = float(np.linalg.norm(g64))
        e_abs = float(np.linalg.norm(grads[name].cpu().numpy().astype(np.float64) - g64))
        if n <= 1e-3 * big:
            assert e_abs <= 5e-6 * big, (name, e_abs, big)
            continue
        e_ora = float(np.linalg.norm(r32["grads"][name].numpy().astype(np.float64) - g64)) / n
        rows.append((e_abs / n, e_ora, name))
    rows.sort(reverse=True)
    import sys
    print("frozen-statistics step vs fp64, %s: engine median %.2e worst %.2e (%s); oracle32 median %.2e worst %.2e" % (
        backbone, sorted(r[0] for r in rows)[len(rows) // 2], rows[0][0], rows[0][2],
        sorted(r[1] for r in rows)[len(rows) // 2], max(r[1] for r in rows)), file=sys.stderr)
    assert rows[0][0] <= 5e-3, rows[0]
    top = "resnet_v2_50/block4/unit_3/" if backbone == "resnet_v2_50" else "InceptionV3/Mixed_7c/Branch_0/"
    tops = [r for r in rows if r[2].startswith(top) or r[2].startswith("dense_")]
    assert tops and max(r[0] for r in tops) <= 1e-4, tops[:3]


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 107, 16, 2), ("resnet_v2_50", 64, 16, 2)])
def test_training_step_against_an_fp64_arbiter(backbone, size, N, V, math="bf16x3"):
    """Which side moves?  The reference's gradient is only defined up to fp32 rounding, and through ~50 train-mode
    BatchNorm layers of a randomly initialised network that rounding is amplified: the CPU oracle evaluated in fp32
    and the SAME oracle evaluated in fp64 differ by 1-3 % per gradient tensor (norm-wise; independent of the number of
    samples per BatchNorm group: measured with 4, 16 and 32 shapes).  north_star's 1e-3 is therefore not a property any
    fp32 implementation of this step can have — TensorFlow's included.  What CAN be demanded: with the fp64 oracle as
    arbiter, the engine must be as close to the truth as the fp32 oracle is.  Per gradient tensor
    |g_engine - g_64| <= 1.5 * |g_oracle32 - g_64| + floor * |g_64|, over the whole gradient vector the engine's error
    is at most 1.25x the fp32 oracle's (measured: 2.4 % vs 2.8 % on Inception-v3 — the engine's fp64 BatchNorm sums
    make it the closer of the two), and loss / logits / shape descriptor agree with fp64 to 1e-4.  The floor covers the
    top-most layers, where the oracle's fp32 is still ~1e-4 from fp64 but ONE flipped ReLU mask among the 64 samples of
    a (view, channel) BatchNorm group already moves that channel's gradient by ~1 %: floor = 1e-2 (the training engine
    evaluates fp32 through bf16 planes: its forward is ~1e-6 from fp64 instead of the oracle's ~1e-7, so more values
    sit within rounding distance of a ReLU threshold; measured worst case 0.8 % on Mixed_7c)."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    shapes = eng.plan.param_shapes()
    P = gv.params.init_backbone_params(shapes, seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, math=math)
    floor = 2e-3 if math == "f32" else 1e-2
    x = torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5
    labels = torch.arange(N) % C_
    r32 = OT.loss_and_grads(x, labels.numpy(), P, Hd, G, backbone)
    r64 = OT.loss_and_grads(x.double(), labels.numpy(), {k: torch.as_tensor(v).double() for k, v in P.items()},
                            {k: torch.as_tensor(v).double() for k, v in Hd.items()}, G, backbone)
    assert r32["scheme"].tolist() == r64["scheme"].tolist()
    scores, S, logits, loss = eng.forward(x.to(DEV), labels)
    assert eng.scheme.cpu().numpy().tolist() == r64["scheme"].tolist()
    close(S.cpu(), r64["shape_descriptor"], 1e-4)
    close(logits.cpu(), r64["logits"], 1e-4)
    assert abs(float(loss) - r64["loss"]) <= 1e-4 * max(1.0, abs(r64["loss"]))
    grads = eng.backward()
    torch.cuda.synchronize()
    tot_e = tot_o = tot_n = 0.0
    rows = []
    big = max(float(g.norm()) for g in r64["grads"].values())
    for name, g64 in r64["grads"].items():
        g64 = g64.numpy()
        n = float(np.linalg.norm(g64))
        e_eng = float(np.linalg.norm(grads[name].cpu().numpy().astype(np.float64) - g64))
        e_ora = float(np.linalg.norm(r32["grads"][name].numpy().astype(np.float64) - g64))
        tot_e += e_eng ** 2
        tot_o += e_ora ** 2
        tot_n += n ** 2
        rows.append((e_eng / max(n, 1e-30), e_ora / max(n, 1e-30), n / big, name))
    import sys
    for r in sorted(rows, reverse=True)[:12]:
        print("ARB %.4f %.4f %.3g %s" % r, file=sys.stderr)
    print("ARB total engine %.5f oracle32 %.5f" % (tot_e ** 0.5 / tot_n ** 0.5, tot_o ** 0.5 / tot_n ** 0.5), file=sys.stderr)
    for e_rel, o_rel, w, name in rows:
        assert e_rel <= 1.5 * o_rel + floor + 1e-5 / max(w, 1e-30), (name, e_rel, o_rel)
    assert tot_e ** 0.5 <= 1.25 * tot_o ** 0.5, (tot_e ** 0.5 / tot_n ** 0.5, tot_o ** 0.5 / tot_n ** 0.5)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_resnet_bias_gradients_known_without_a_pass(storage):
    """TrainGVCNN._bias_sources: in train mode 19 of ResNet-v2-50's 21 bias gradients need no pass over dy — a bias in front of
    a train-mode BatchNorm (conv1 through pool1, the last conv3 of blocks 1 and 2) has a ZERO gradient, and a bias behind a
    residual add has the gradient of the add's own bias (nets/resnet_v2.py:79-91: every other conv3 and the four shortcut
    convolutions).  (1) The mathematics, on the oracle's fp64 autograd: the zeros are zero and the copies equal to 1e-6 of
    the largest bias gradient.  (2) The engine with the identities reproduces exactly that structure (zeros are 0.0, copies
    bit-equal, the two summed biases bit-equal to the engine that sums all 21) and (3), on fp32 storage, the engine that sums
    all 21 agrees with it to 2e-3 of the largest bias gradient.  With frozen statistics only the four residual twins remain."""
    backbone, N, V, size, C_, G = "resnet_v2_50", 4, 2, 64, 5, 10
    probe = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(probe.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, probe.raw.c, probe.final.c, C_, seed=3, spread_scores=True)
    del probe
    x = torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5
    labels = torch.arange(N) % C_
    r64 = OT.loss_and_grads(x.double(), labels.numpy(), {k: torch.as_tensor(v).double() for k, v in P.items()},
                            {k: torch.as_tensor(v).double() for k, v in Hd.items()}, G, backbone)
    out = {}
    for on in (True, False):
        eng = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage=storage)
        eng.bias_grad_identities = on
        eng.forward(x.to(DEV), labels)
        out[on] = {k: v.clone().cpu().double() for k, v in eng.backward().items() if k.endswith("/biases")}
        if on:
            src = eng._bias_sources()
    assert sorted(src) == sorted(out[True]) and len(src) == 21
    assert sum(v is None for v in src.values()) == 2 and sum(v == [] for v in src.values()) == 3
    big = max(float(r64["grads"][k].abs().max()) for k in src)
    # (3) only on fp32 storage: the sum of 16-bit stored dy values carries rounding noise of the order of the largest true
    # bias gradient itself (measured > 0.2 of it on conv1) — the summed form is the LESS accurate of the two there
    noise = 2e-3 if storage == "f32" else float("inf")
    for name, s_ in src.items():
        g64 = r64["grads"][name].double()
        if s_ is None:
            assert torch.equal(out[True][name], out[False][name]), name
        elif s_ == []:
            assert float(g64.abs().max()) <= 1e-6 * big, (name, float(g64.abs().max()), big)
            assert float(out[True][name].abs().max()) == 0.0, name
            assert float(out[False][name].abs().max()) <= noise * big, (name, float(out[False][name].abs().max()), big)
        else:
            assert len(s_) == 1
            assert float((g64 - r64["grads"][s_[0]].double()).abs().max()) <= 1e-6 * big, name
            assert torch.equal(out[True][name], out[True][s_[0]]), name
            assert float((out[False][name] - out[True][name]).abs().max()) <= noise * big, name
    frozen = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage=storage,
                        frozen_bn=True)
    fs = frozen._bias_sources()
    assert sum(v is None for v in fs.values()) == 17 and all(v is None or (len(v) == 1 and "/shortcut/" in k) for k, v in fs.items())


@pytest.mark.parametrize("backbone,size", [("inception_v3", 171), ("resnet_v2_50", 129)])
def test_gradient_is_the_directional_derivative_of_the_loss(backbone, size):
    """Oracle-free check of the assembled backward pass: along the gradient direction the loss must change by
    |g| per unit step: (L(w + e*g/|g|) - L(w - e*g/|g|)) / 2e  ==  |g|   (central difference, fixed grouping)."""
    N, V, C_, G = 4, 2, 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=5, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=6, spread_scores=True)
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    labels = torch.tensor([0, 3, 1, 2])
    eng.forward(x, labels)
    scheme, weight = eng.scheme.cpu().numpy().copy(), eng.weight.cpu().numpy().copy()
    grads = {k: v.clone() for k, v in eng.backward().items()}
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    w0 = {k: eng.params[k].clone() for k in grads}
    def central(eps):
        L = []
        for sgn in (+1.0, -1.0):
            for k in grads:
                eng.params[k].copy_(w0[k] + sgn * eps * grads[k] / gnorm)
            eng._packed_dirty = True
            L.append(float(eng.forward(x, labels, g_scheme=scheme, g_weight=weight)[3]))
        return (L[0] - L[1]) / (2 * eps)

    # train-mode BN over few samples makes the loss strongly curved: Richardson-extrapolate the
    # O(eps^2) error of the central difference away
    d1, d2 = central(1e-4), central(2e-4)
    deriv = (4 * d1 - d2) / 3
    assert abs(deriv - gnorm) <= 2e-2 * gnorm, (d1, d2, deriv, gnorm)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_view_sharded_engines_reproduce_the_whole_step(storage):
    """sharding.ShardedTrainGVCNN's algorithm on ONE device: two engines own views {0,1} and {2,3} (per-view
    BatchNorm statistics stay inside an engine), the gather along the view axis is a torch.cat, every
    engine runs the head on the gathered data, takes its slice of dF, and the backbone gradients of the
    two engines are added — equal to the unsharded engine's step.  bf16 storage: with one fixed tile configuration
    (the heuristic's choice depends on the number of images, and a different summation order inside a tile moves
    bf16 roundings, which the train-mode network then amplifies) every per-view tensor is bit-identical in the
    sharded and the unsharded run, so the same tolerance holds."""
    if storage != "f32":
        lib().gv_conv2d_set_tile_override(0)
    try:
        _view_sharded_step(storage)
    finally:
        lib().gv_conv2d_set_tile_override(-1)


def _view_sharded_step(storage):
    backbone, size, N, V, C_, G = "resnet_v2_50", 97, 3, 4, 5, 10
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(full.plan.param_shapes(), seed=5, perturb_bn=True)
    Hd = gv.params.init_head_params(V, full.raw.c, full.final.c, C_, seed=6, spread_scores=True)
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage=storage)
    # The separate statistics passes sum every view over ITS pixels in a fixed split, whatever the engine's view count:
    # sharded and unsharded engines are then bit-identical per view and this test can hold the fp32 tolerance on 16-bit
    # storage too.  The sums folded into the convolution epilogues (fuse_bn_stats) are grouped by row tile, i.e. they
    # depend on how the views interleave in the batch: equal to summation order only (test_gpu_bn_fusion.py), which the
    # train-mode statistics of a random network then amplify.
    full.fuse_bn_stats = False
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    labels = torch.tensor([0, 3, 1])
    full.forward(x, labels)
    ref = {k: v.clone() for k, v in full.backward().items()}
    Vl = V // 2
    engs = [TrainGVCNN(backbone, N, Vl, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV,
                       head_views=V, view_offset=r * Vl, storage=storage) for r in range(2)]
    for e in engs:
        e.fuse_bn_stats = False
    f = engs[0].final
    for r, e in enumerate(engs):
        e.forward_backbone(x[:, r * Vl:(r + 1) * Vl].contiguous())
    r_all = torch.cat([e.score_partial().view(N, Vl) for e in engs], dim=1).contiguous()
    F_all = torch.cat([e.view(f).view(N, Vl, f.h, f.w, f.c) for e in engs], dim=1).contiguous()
    total = None
    for r, e in enumerate(engs):
        _, S, logits, loss = e.forward_head(labels, F=F_all, r_img=r_all.reshape(-1))
        close(loss.cpu(), full.loss.cpu(), 1e-5)
        assert e.scheme.cpu().tolist() == full.scheme.cpu().tolist()
        dF = torch.zeros_like(F_all)
        e.backward_head(dF=dF)
        e.final_grad().copy_(dF[:, r * Vl:(r + 1) * Vl])
        g = e.backward_backbone()
        if total is None:
            total = {k: v.clone() for k, v in g.items()}
        else:
            for k, v in g.items():
                if k not in e.cls_names:
                    total[k] += v
    gmax = max(float(v.abs().max()) for v in ref.values())
    for k, r_ in ref.items():
        scale = float(r_.abs().max())
        err = float((total[k] - r_).abs().max())
        if scale < 1e-5 * gmax:
            assert err < 1e-5 * gmax, k                  # bias in front of a train-mode BN: zero gradient
        else:
            assert err < 2e-4 * scale, (k, err, scale)   # same kernels; only atomic summation order differs


@pytest.mark.parametrize("backbone,size", [("inception_v3", 107), ("resnet_v2_50", 64)])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_backward_progress_frontier_is_final(backbone, size, storage):
    """backward_backbone(progress=cb): when cb(lo) is called, the filter-gradient region flat_g[lo:n_wd] must already hold
    its FINAL values (stream order) — nothing enqueued later writes it.  That is what lets a data-parallel wrapper start
    all-reducing that slice while the rest of the backward pass runs (sharding.OverlappedFlatAllReduce).  Checked by
    snapshotting the region at every call (a device-side copy on the same stream) and comparing with the end of the pass;
    the frontier must also reach 0 and shrink monotonically, and every '/weights' gradient must lie inside the region."""
    N, V, C_, G = 2, 2, 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV, storage=storage)
    assert eng._g_monotone
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    eng.forward(x, torch.tensor([1, 3]))
    eng.backward_head()
    snaps, los = [], []

    def cb(lo):
        los.append(lo)
        if len(snaps) < 12 or lo == 0:                       # a dozen early frontiers + the last one
            snaps.append((lo, eng._flat_g[lo:eng._n_wd].clone()))
    eng.backward_backbone(progress=cb)
    torch.cuda.synchronize()
    assert los and los[-1] == 0 and all(a > b for a, b in zip(los, los[1:]))
    for lo, snap in snaps:
        assert torch.equal(snap, eng._flat_g[lo:eng._n_wd]), lo
    base = eng._flat_g.data_ptr()
    for k, g in eng.grads.items():
        inside = 0 <= (g.data_ptr() - base) // 4 < eng._n_wd
        assert inside == k.endswith("/weights"), k


def test_bn_moving_average_update():
    """UPDATE_OPS of train.py:178-186: V sequential updates with the unbiased variance; and end to end through
    TrainGVCNN (moving statistics after one step == oracle formula on the engine's own batch statistics)."""
    from oracle import train as OT
    g = torch.Generator().manual_seed(4)
    V, c = 5, 70
    mean, var = torch.randn(V, c, generator=g), torch.rand(V, c, generator=g) + 0.1
    mm, mv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    counts = torch.tensor([12, 12, 7, 1, 30], dtype=torch.int32)
    md, vd, cd, mmd, mvd = mean.to(DEV), var.to(DEV), counts.to(DEV), mm.to(DEV), mv.to(DEV)
    _lib.check(lib().gv_bn_update_moving(md.data_ptr(), vd.data_ptr(), cd.data_ptr(), V, c, 0.997, mmd.data_ptr(),
                                         mvd.data_ptr(), st()), "bn_update_moving")
    omm, omv = OT.moving_average_update(mm.numpy(), mv.numpy(), mean.numpy(), var.numpy(), counts.numpy(), 0.997)
    np.testing.assert_allclose(mmd.cpu().numpy(), omm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(mvd.cpu().numpy(), omv, rtol=1e-6, atol=1e-7)
    # through the engine
    eng = TrainGVCNN("resnet_v2_50", 2, 2, 64, 64, 5, 10, device=DEV)
    x = (torch.rand(2, 2, 64, 64, 3, generator=g) - 0.5).to(DEV)
    name = "resnet_v2_50/block1/unit_1/bottleneck_v2/preact"
    mm0 = eng.params[name + "/moving_mean"].clone()
    mv0 = eng.params[name + "/moving_variance"].clone()
    eng.train_step(x, torch.tensor([1, 2]), lr=0.0)
    op = [o for o in eng.plan.ops if o["kind"] == "bn" and o["name"] == name][0]
    n = 2 * op["x"].h * op["x"].w
    omm, omv = OT.moving_average_update(mm0.cpu().numpy(), mv0.cpu().numpy(), op["stat"]["mean"].cpu().numpy(),
                                        op["stat"]["var"].cpu().numpy(), [n, n], 0.997)
    np.testing.assert_allclose(eng.params[name + "/moving_mean"].cpu().numpy(), omm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(eng.params[name + "/moving_variance"].cpu().numpy(), omv, rtol=1e-6, atol=1e-7)
    assert not torch.equal(eng.params[name + "/moving_mean"], mm0)


@pytest.mark.parametrize("weight_mode,pool", [(0, "max"), (1, "max"), (1, "mean")])
def test_per_shape_fuse_backward_vs_autograd(weight_mode, pool):
    """gv_view_pool_fuse_bwd_per_shape: every shape has its own scheme/weights (constants of the backward pass); ties
    split equally; a shape whose weights sum to 0 (mean_score, all scores 0) gets no gradient."""
    rng = np.random.RandomState(5 + weight_mode)
    N, V, G, E = 4, 6, 10, 40
    scores = rng.uniform(0, 0.99, size=(N, V)).astype(np.float32)
    scores[2] = 0.0
    Fh = rng.randn(N, V, E).astype(np.float32)
    Fh[1, 3] = Fh[1, 0]                                         # a full tie between two views of shape 1
    scores[1, 3] = scores[1, 0]                                 # ... in the same group
    dS = rng.randn(N, E).astype(np.float32)
    sd, Fd, dSd = torch.from_numpy(scores).to(DEV), torch.from_numpy(Fh).to(DEV), torch.from_numpy(dS).to(DEV)
    gidx = torch.empty(N, V, dtype=torch.int32, device=DEV)
    scheme = torch.empty(N, G, V, dtype=torch.int32, device=DEV)
    weight = torch.empty(N, G, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib().gv_group_assign_per_shape(sd.data_ptr(), N, V, G, 10, weight_mode, gidx.data_ptr(),
                                               scheme.data_ptr(), weight.data_ptr(), status.data_ptr(), st()), "assign")
    mode = _lib.GV_VIEWPOOL_MAX if pool == "max" else _lib.GV_VIEWPOOL_MEAN
    dF = torch.zeros(N, V, E, device=DEV)
    _lib.check(lib().gv_view_pool_fuse_bwd_per_shape(Fd.data_ptr(), dSd.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(),
                                                     G, weight.data_ptr(), mode, dF.data_ptr(), st()), "bwd")
    # autograd through the oracle-shaped forward, shape by shape
    Ft = torch.from_numpy(Fh).requires_grad_(True)
    sch, w = scheme.cpu().numpy(), weight.cpu().numpy()
    total = 0.0
    for n in range(N):
        if float(w[n].sum()) == 0.0:
            continue
        acc = 0.0
        for g in range(G):
            idx = np.nonzero(sch[n, g])[0]
            if idx.size == 0:
                d = torch.ones(E)
            elif pool == "max":
                d = torch.amax(Ft[n, torch.as_tensor(idx)], dim=0)
            else:
                d = Ft[n, torch.as_tensor(idx)].mean(dim=0)
            acc = acc + float(w[n, g]) * d
        total = total + ((acc / float(w[n].sum())) * torch.from_numpy(dS[n])).sum()
    total.backward()
    close(dF.cpu(), Ft.grad, 1e-5)
    if weight_mode == 1:
        assert float(dF[2].abs().max()) == 0.0


def test_training_engine_with_per_shape_grouping():
    """TrainGVCNN(per_shape=True): the head is the per-shape module (checked against the oracle on the engine's own
    descriptors / responses) and the backward pass runs through it."""
    from oracle import grouping as OG
    N, V, C_, G = 3, 4, 5, 10
    eng = TrainGVCNN("resnet_v2_50", N, V, 64, 64, C_, G, device=DEV, per_shape=True, weight_mode="mean_score")
    x = (torch.rand(N, V, 64, 64, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    scores, S, logits, loss = eng.forward(x, torch.tensor([0, 1, 2]))
    f = eng.final
    Fh = eng.view(f).view(N, V, f.h, f.w, f.c).cpu().numpy()
    o_scores, o_sch, o_w, o_S = OG.per_shape_grouping(Fh, eng.r_img.cpu().numpy().reshape(N, V), G, weight_mode="mean_score")
    np.testing.assert_allclose(scores.cpu().numpy(), o_scores, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(S.cpu().numpy(), o_S, rtol=1e-5, atol=1e-5 * float(np.abs(o_S).max()))
    grads = eng.backward()
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    assert np.isfinite(float(loss)) and np.isfinite(gn) and gn > 0


def test_shape_sharded_engines_reproduce_the_whole_step():
    """sharding.ShardedTrainGVCNN(mode='shapes') on ONE device: two engines own shapes {0,1} and {2,3} with all their
    views; every BatchNorm's sums are added across the two engines between the two halves of the split entry points
    (the all-reduce), scores are finalised over the global batch, dlogits carry the 1/world factor — gradients, loss
    and BN batch statistics equal the unsharded engine's."""
    import threading
    backbone, size, N, V, C_, G, W_ = "resnet_v2_50", 64, 4, 2, 5, 10, 2
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(full.plan.param_shapes(), seed=5, perturb_bn=True)
    Hd = gv.params.init_head_params(V, full.raw.c, full.final.c, C_, seed=6, spread_scores=True)
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    labels = torch.tensor([0, 3, 1, 2])
    full.forward(x, labels)
    ref = {k: v.clone() for k, v in full.backward().items()}
    Nl = N // W_
    engs = [TrainGVCNN(backbone, Nl, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV) for _ in range(W_)]
    # a two-party "all-reduce" between the engines: each bn_sync call parks its accumulator until the peer arrives
    barrier = threading.Barrier(W_)
    slots = [None] * W_

    def make_sync(r):
        def sync(acc):
            torch.cuda.synchronize()
            slots[r] = acc.clone()
            barrier.wait()
            total = slots[0] + slots[1]
            barrier.wait()
            acc.copy_(total)
        return sync
    for r, e in enumerate(engs):
        e.shape_world = W_
        e.bn_sync = make_sync(r)
    out = [None] * W_
    r_parts = [None] * W_

    def run(r):
        with torch.cuda.device(0):
            e = engs[r]
            e.forward_backbone(x[r * Nl:(r + 1) * Nl].contiguous())
            torch.cuda.synchronize()
            r_parts[r] = e.score_partial().clone()
            torch.cuda.synchronize()
            barrier.wait()
            r_all = torch.cat(r_parts)
            _lib.check(lib().gv_view_score_finalize(r_all.data_ptr(), N, V, _lib.GV_ORDER_SHAPE_MAJOR,
                                                    e.scores.data_ptr(), st()), "finalize")
            e.forward_head(labels[r * Nl:(r + 1) * Nl], scores_ready=True)
            e.backward_head()
            out[r] = {k: v.clone() for k, v in e.backward_backbone().items()}
            torch.cuda.synchronize()
    th = [threading.Thread(target=run, args=(r,)) for r in range(W_)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(o is not None for o in out)
    assert engs[0].scheme.cpu().tolist() == full.scheme.cpu().tolist()
    close((engs[0].loss + engs[1].loss).cpu() / W_, full.loss.cpu(), 1e-5)
    # batch statistics of a deep layer are the global ones on both engines
    name = "resnet_v2_50/block3/unit_2/bottleneck_v2/conv1/BatchNorm"
    fs = [o for o in full.plan.ops if o["kind"] == "bn" and o["name"] == name][0]["stat"]
    for e in engs:
        es = [o for o in e.plan.ops if o["kind"] == "bn" and o["name"] == name][0]["stat"]
        close(es["mean"].cpu(), fs["mean"].cpu(), 1e-4)
        close(es["var"].cpu(), fs["var"].cpu(), 1e-4)
    gmax = max(float(v.abs().max()) for v in ref.values())
    for k, r_ in ref.items():
        if k.endswith(("/beta", "/gamma")):
            got = out[0][k]                              # already global on every engine
            close(out[1][k].cpu(), out[0][k].cpu(), 1e-5)
        else:
            got = out[0][k] + out[1][k]
        scale = float(r_.abs().max())
        err = float((got - r_).abs().max())
        if scale < 1e-5 * gmax:
            assert err < 1e-5 * gmax, k
        else:
            assert err < 1e-3 * scale, (k, err, scale)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_trainer_checkpoint_resumes_the_run(tmp_path, storage):
    """Trainer.save / restore (tf.train.Saver's role): a run restored from its checkpoint-v2 bundle — variables, BN
    moving statistics, Momentum slots, scorer layers, global step — takes the same next step as the run that wrote it."""
    from gvcnn_tf_amd.trainer import Trainer
    N, V, size, C_, G = 2, 2, 64, 5, 10
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    labels = torch.tensor([1, 3]).to(DEV)
    eng = TrainGVCNN("resnet_v2_50", N, V, size, size, C_, G, device=DEV, seed=7, storage=storage)
    tr = Trainer(eng, base_learning_rate=1e-3, training_number_of_steps=50, check_every=0)
    tr.step(x, labels)
    tr.step(x, labels)
    prefix = str(tmp_path / "model.ckpt-2")
    tr.save(prefix)
    want = float(tr.step(x, labels))
    eng2 = TrainGVCNN("resnet_v2_50", N, V, size, size, C_, G, device=DEV, seed=99, storage=storage)   # other values
    tr2 = Trainer(eng2, base_learning_rate=1e-3, training_number_of_steps=50, check_every=0)
    assert Trainer.latest_checkpoint(str(tmp_path)) == prefix          # the `checkpoint` state file (tf.train.latest_checkpoint)
    assert open(str(tmp_path / "checkpoint")).read().splitlines()[0] == 'model_checkpoint_path: "model.ckpt-2"'
    assert tr2.restore(prefix) == [] and tr2.global_step == 2
    got = float(tr2.step(x, labels))
    assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (got, want)
    tol = 1e-4 if storage == "f32" else 2e-2             # (fp32 atomics in the filter gradient; bf16 roundings on top)
    for k in eng.params:                                 # and lands on the same variables
        a, b = eng2.params[k].float().cpu(), eng.params[k].float().cpu()
        assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-3), k


def test_out_of_range_label_is_nan_not_an_out_of_bounds_read():
    """a label outside [0, C) — or an int64 that does not fit an int — must never index the logits.
    Like TensorFlow's GPU kernel the row's loss and gradient become NaN; the other rows keep their values and the
    trainer's check_numerics emulation (train.py:175) raises."""
    import ctypes as C_
    from gvcnn_tf_amd import _lib
    lib = _lib.load()
    n, c = 5, 7
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(n, c, generator=g).to(DEV)
    labels = torch.tensor([1, 6, 0, 3, 2], dtype=torch.int64)
    loss = torch.zeros(1, device=DEV)
    dl = torch.zeros(n, c, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gv_softmax_ce(logits.data_ptr(), labels.to(DEV).data_ptr(), n, c, loss.data_ptr(), dl.data_ptr(), st), "ce")
    want = torch.nn.functional.cross_entropy(logits.cpu(), labels)
    assert abs(float(loss.item()) - float(want)) < 1e-6
    good = dl.cpu().clone()
    for bad in (7, -1, 2 ** 32 + 1, 2 ** 40):
        lb = labels.clone()
        lb[3] = bad
        _lib.check(lib.gv_softmax_ce(logits.data_ptr(), lb.to(DEV).data_ptr(), n, c, loss.data_ptr(), dl.data_ptr(), st), "ce")
        assert math.isnan(float(loss.item())), bad
        d = dl.cpu()
        assert torch.isnan(d[3]).all() and torch.equal(d[[0, 1, 2, 4]], good[[0, 1, 2, 4]]), bad


def test_trainer_raises_like_the_host_group_scheme_on_a_score_of_one():
    """a view score of exactly 1.0 (bin == num_group) leaves that view in no group while the loss
    stays finite; the reference's host group_scheme raises IndexError there (nets/model.py:23 via train.py:277).
    Trainer.step reads the status word of the step in its check."""
    from gvcnn_tf_amd.trainer import Trainer
    N, V, size, C_, G = 2, 2, 64, 5, 10
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    labels = torch.tensor([1, 3]).to(DEV)
    eng = TrainGVCNN("resnet_v2_50", N, V, size, size, C_, G, device=DEV, seed=7)
    tr = Trainer(eng, base_learning_rate=1e-4, training_number_of_steps=50, check_every=1)
    tr.step(x, labels)                                            # fine
    eng.score_bias[0] = 1e9                                       # |r| >= 3e7 rounds sigmoid(log|r|) to exactly 1.0f
    with pytest.raises(IndexError, match="index 10 is out of bounds for axis 0 with size 10"):
        tr.step(x, labels)


def test_hybrid_sharded_engines_reproduce_the_whole_step():
    """sharding.ShardedTrainGVCNN(mode='hybrid') emulated on ONE device: 2 view groups x 2 shape shards = four engines,
    each owning half the views of half the shapes (the layout that gives 8 GPUs 3 of 12 views of half the batch each).
    BatchNorm sums are added inside a shape group (same views), descriptors gathered inside a view group (same shapes),
    scores finalised over the whole [N, V] array; variable gradients summed over all four, beta/gamma over the two view
    groups, the classifier over the two shape shards — and everything equals the unsharded engine's step."""
    import threading
    backbone, size, N, V, C_, G = "resnet_v2_50", 64, 4, 4, 5, 10
    VG, SH = 2, 2
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(full.plan.param_shapes(), seed=5, perturb_bn=True)
    Hd = gv.params.init_head_params(V, full.raw.c, full.final.c, C_, seed=6, spread_scores=True)
    full = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    labels = torch.tensor([0, 3, 1, 2])
    full.forward(x, labels)
    ref = {k: v.clone() for k, v in full.backward().items()}
    Nl, Vl = N // SH, V // VG
    engs = {(g, k): TrainGVCNN(backbone, Nl, Vl, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV,
                               head_views=V, view_offset=g * Vl) for g in range(VG) for k in range(SH)}
    bar_all = threading.Barrier(VG * SH)
    bar_shape = {g: threading.Barrier(SH) for g in range(VG)}
    slots = {}

    def make_sync(g, k):                               # the all-reduce inside shape group g
        def sync(acc):
            torch.cuda.synchronize()
            slots[("bn", g, k)] = acc.clone()
            bar_shape[g].wait()
            total = slots[("bn", g, 0)] + slots[("bn", g, 1)]
            bar_shape[g].wait()
            acc.copy_(total)
        return sync
    for (g, k), e in engs.items():
        e.shape_world = SH
        e.bn_sync = make_sync(g, k)
    out, errors = {}, []

    def run(g, k):
        try:
            with torch.cuda.device(0):
                e = engs[(g, k)]
                f = e.final
                xs = x[k * Nl:(k + 1) * Nl, g * Vl:(g + 1) * Vl].contiguous()
                e.forward_backbone(xs)
                torch.cuda.synchronize()
                slots[("r", g, k)] = e.score_partial().view(Nl, Vl).clone()
                slots[("F", g, k)] = e.view(f).view(Nl, Vl, f.h, f.w, f.c).clone()
                torch.cuda.synchronize()
                bar_all.wait()
                r_views = torch.cat([slots[("r", gg, k)] for gg in range(VG)], dim=1)                    # view group gather
                r_all = torch.cat([torch.cat([slots[("r", gg, kk)] for gg in range(VG)], dim=1) for kk in range(SH)], dim=0)
                F_all = torch.cat([slots[("F", gg, k)] for gg in range(VG)], dim=1).contiguous()
                _lib.check(lib().gv_view_score_finalize(r_all.contiguous().data_ptr(), N, V, _lib.GV_ORDER_SHAPE_MAJOR,
                                                        e.scores.data_ptr(), st()), "finalize")
                e.forward_head(labels[k * Nl:(k + 1) * Nl], F=F_all, r_img=r_views.contiguous().reshape(-1), scores_ready=True)
                dF = torch.zeros_like(F_all)
                e.backward_head(dF=dF)
                e.final_grad().copy_(dF[:, g * Vl:(g + 1) * Vl])
                out[(g, k)] = {n: v.clone() for n, v in e.backward_backbone().items()}
                torch.cuda.synchronize()
        except Exception as ex:                        # a dead thread must not leave the others at a barrier
            errors.append(ex)
            bar_all.abort()
            for b_ in bar_shape.values():
                b_.abort()
    th = [threading.Thread(target=run, args=gk) for gk in engs]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert all(engs[gk].scheme.cpu().tolist() == full.scheme.cpu().tolist() for gk in engs)
    close(sum(engs[(0, k)].loss for k in range(SH)).cpu() / SH, full.loss.cpu(), 1e-5)
    gmax = max(float(v.abs().max()) for v in ref.values())
    cls = set(full.cls_names)
    for name, r_ in ref.items():
        if name.endswith(("/beta", "/gamma")):          # summed over the shapes by the BatchNorm exchange: view groups add up
            got = out[(0, 0)][name] + out[(1, 0)][name]
            close(out[(0, 1)][name].cpu(), out[(0, 0)][name].cpu(), 1e-5)
        elif name in cls:                               # identical inside a view group: shape shards add up
            got = out[(0, 0)][name] + out[(0, 1)][name]
            close(out[(1, 0)][name].cpu(), out[(0, 0)][name].cpu(), 1e-5)
        else:
            got = sum(out[gk][name] for gk in engs)
        scale = float(r_.abs().max())
        err = float((got - r_).abs().max())
        if scale < 1e-5 * gmax:
            assert err < 1e-5 * gmax, name
        else:
            assert err <= 2e-4 * scale, (name, err / scale)
