"""Training the grouping module (TrainGVCNN(train_scorer=True)): the two scorer-gradient entry points of
csrc/scorer_bwd.hip against the fp64 autograd reference of tests/scorer_ref.py, then the engine — forward untouched,
gradients above the raw tap untouched, scorer gradients against the reference on the engine's own taps, the term that
enters the trunk, steps, refusals and checkpoints.

Tolerances.  A gradient here is a sum of terms of both signs (dw is a difference of near-equal quantities when one
group dominates), so fp32 results are held to 1e-5 of their ABSOLUTE-term sums (the `close(.., 1e-5)` rule of
test_gpu_train.py::test_per_shape_fuse_backward_vs_autograd, taken term-wise); the raw-tap term is one product per
element: 1e-6 of |destination| + |term| in fp32, one rounding of the storage type (2^-8 / 2^-11 relative, the constants
of test_gpu_train_lp.py::TYPES; below the type's normal range: half its subnormal spacing) on 16-bit storage.

Engine seeds: backbone seed 2, head seed 3 with spread_scores=True, batch seed 3.  spread_scores puts the V scorer biases
on distinct score bins, so every shape has V non-empty groups whatever the batch; the tests assert that from gidx_ps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib, backbones           # noqa: E402
from gvcnn_tf_amd import params as gparams         # noqa: E402
from gvcnn_tf_amd.trainer import Trainer           # noqa: E402
from gvcnn_tf_amd.training import TrainGVCNN, TrainPlan   # noqa: E402

import scorer_ref as R                             # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
# (dtype code, torch dtype, relative bound of one rounding, half the subnormal spacing)
STORAGE = {"f32": (_lib.GV_F32, torch.float32, None, 0.0),
           "bf16": (_lib.GV_BF16, torch.bfloat16, 2.0 ** -8, 2.0 ** -134),
           "f16": (_lib.GV_F16, torch.float16, 2.0 ** -11, 2.0 ** -25)}
G = 10


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def assert_within(dev, ref, bound, what):
    dev, ref, bound = dev.detach().cpu().to(F64), ref.to(F64), bound.to(F64)
    err = (dev - ref).abs()
    worst = float((err - bound).max())
    print("%s: max|dev - ref| = %.3e, max bound = %.3e, max(err - bound) = %.3e"
          % (what, float(err.max()), float(bound.max()), worst))
    assert bool(torch.isfinite(dev).all()), what
    assert bool((err <= bound).all()), "%s: error exceeds its bound by %.3e" % (what, worst)


# ---- 1. dL/dw -------------------------------------------------------------------------------------------------------
def _dw_fixture(E, tdt):
    rng = np.random.RandomState(11)
    N, V = 4, 6
    scores = rng.uniform(0.0, 0.99, size=(N, V)).astype(np.float32)
    scores[1, 3] = scores[1, 0]                                 # two views of shape 1 in one group ...
    scores[2] = 0.0                                             # every weight of shape 2 is 0: W = 0
    scores[3] = np.linspace(0.51, 0.58, V, dtype=np.float32)    # every view of shape 3 in group 5
    Fh = torch.from_numpy(rng.randn(N, V, E).astype(np.float32)).to(tdt)
    Fh[1, 3] = Fh[1, 0]                                         # ... with equal descriptors: a full tie
    dS = torch.from_numpy(rng.randn(N, E).astype(np.float32))
    return N, V, torch.from_numpy(scores), Fh, dS


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("E", [96, 63, 5000])
@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
def test_group_weight_gradient_vs_autograd(storage, E, pool):
    """gv_group_weight_bwd_per_shape: 96 = one vector chunk, 63 = the scalar path, 5000 = several chunks and a ragged
    last one.  Shape 2 (W = 0) and every empty group get exactly 0; two calls give the same bits."""
    dt, tdt, _, _ = STORAGE[storage]
    N, V, scores, Fh, dS = _dw_fixture(E, tdt)
    sd, Fd, dSd = scores.to(DEV), Fh.to(DEV), dS.to(DEV)
    gidx = torch.empty(N, V, dtype=torch.int32, device=DEV)
    scheme = torch.empty(N, G, V, dtype=torch.int32, device=DEV)
    weight = torch.empty(N, G, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib().gv_group_assign_per_shape(sd.data_ptr(), N, V, G, 10, _lib.GV_WEIGHT_MEAN_SCORE, gidx.data_ptr(),
                                               scheme.data_ptr(), weight.data_ptr(), status.data_ptr(), st()), "assign")
    nws = lib().gv_group_weight_bwd_workspace_bytes(N, E, G)
    assert nws > 0
    mode = _lib.GV_VIEWPOOL_MAX if pool == "max" else _lib.GV_VIEWPOOL_MEAN
    outs = []
    for fill in (1.0, -3.0):                                    # (whatever the outputs and the workspace held before)
        ws = torch.full((nws // 4,), fill, device=DEV)
        dw = torch.full((N, G), fill, device=DEV)
        _lib.check(lib().gv_group_weight_bwd_per_shape(Fd.data_ptr(), dSd.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(),
                                                       G, weight.data_ptr(), mode, dw.data_ptr(), ws.data_ptr(), nws, dt,
                                                       st()), "group_weight_bwd")
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    gi = gidx.cpu()
    assert int(status.item()) == 0 and len(set(gi[3].tolist())) == 1 and int(gi[1, 0]) == int(gi[1, 3])
    ref, A = R.group_weight_grad(Fh.to(F64), dS.to(F64), gi, weight.cpu().to(F64), G, pool)
    assert_within(outs[0], ref, 1e-5 * A, "dw %s E=%d %s" % (storage, E, pool))
    _, cnt = R.members(gi, G)
    assert float(outs[0][2].abs().max()) == 0.0                 # W = 0
    assert float(outs[0][cnt == 0].abs().max()) == 0.0          # empty groups
    assert float(outs[0][0].abs().max()) > 0.0 and float(outs[0][1].abs().max()) > 0.0


# ---- 2. scorer backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cr,pad", [(24, 0), (24, 8), (7, 0), (7, 8)])
@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
def test_scorer_backward_vs_autograd(storage, cr, pad, accumulate):
    """gv_view_score_bwd: dkernel, dbias and the raw-tap term; raw and its gradient as channel slices (raw_ld = cr + 8),
    a negative response, an exact 0, a view in no group; the columns past cr keep their sentinel."""
    _scorer_backward_case(storage, cr, pad, accumulate, 3, 4, 4)


@pytest.mark.parametrize("N,V,hw,cr,pad", [(3, 4, 289, 24, 8), (3, 4, 131, 7, 0), (260, 2, 4, 8, 0)])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_scorer_backward_at_production_map_sizes(storage, N, V, hw, cr, pad):
    """The same at the sizes where the filter-gradient kernel takes its other loops: hw = 289 (Mixed_6e at 224 x 224) and
    131 run the four-loads-in-flight pixel loop and its tail, 260 shapes a second tile of the per-shape responses."""
    _scorer_backward_case(storage, cr, pad, 0, N, V, hw)


def _scorer_backward_case(storage, cr, pad, accumulate, N, V, hw):
    dt, tdt, eps, tiny = STORAGE[storage]
    ld = cr + pad
    g = torch.Generator().manual_seed(100 + cr + pad)
    r_img = torch.randn(N, V, generator=g) * 1.5
    r_img[0, 0], r_img[0, V - 1] = 0.55, -0.6                   # scores 0.355 and 0.375: one group, one of them r < 0
    r_img[1, V - 1] = 0.0                                       # s = 0: dr = 0 there
    s = (r_img.abs() / (1 + r_img.abs())).float()
    gidx = (s * np.float32(10)).to(torch.int32)
    gidx[2, 0] = G                                              # in no group (status bit 1 of the assignment)
    assert int(gidx[0, 0]) == int(gidx[0, V - 1]) == 3 and bool((r_img < 0).any())
    dw = torch.randn(N, G, generator=g)
    kernel = torch.randn(V, cr, generator=g) * 0.3
    raw = torch.randn(N * V, hw, cr, generator=g).to(tdt)
    SENT = 7.0
    rawbuf = torch.full((N * V, hw, ld), SENT, dtype=tdt)
    rawbuf[:, :, :cr] = raw
    dst = torch.randn(N * V, hw, cr, generator=g).to(tdt) if accumulate else torch.full((N * V, hw, cr), -5.0, dtype=tdt)
    dbuf = torch.full((N * V, hw, ld), SENT, dtype=tdt)
    dbuf[:, :, :cr] = dst
    rd, dd = rawbuf.to(DEV), dbuf.to(DEV)
    dk, db = torch.full((V, cr), 9.0, device=DEV), torch.full((V,), 9.0, device=DEV)
    kd, rid, gid, dwd = kernel.to(DEV), r_img.reshape(-1).to(DEV), gidx.to(DEV), dw.to(DEV)   # (kept alive over the call)
    _lib.check(lib().gv_view_score_bwd(rd.data_ptr(), N * V, hw, cr, ld, kd.data_ptr(), rid.data_ptr(), gid.data_ptr(),
                                       dwd.data_ptr(), G, V, dk.data_ptr(), db.data_ptr(), dd.data_ptr(), ld, accumulate,
                                       dt, st()), "view_score_bwd")
    torch.cuda.synchronize()
    dr, dr_abs = R.response_grad(r_img.to(F64), gidx, dw.to(F64), G)
    assert float(dr[1, V - 1]) == 0.0 and float(dr[2, 0]) == 0.0 and float(dr[0, V - 1]) != 0.0
    rk, rb, term, A_k, A_b = R.scorer_grad(raw.to(F64).reshape(N, V, hw, cr), kernel.to(F64), dr, dr_abs)
    what = "%s N=%d V=%d hw=%d cr=%d ld=%d acc=%d" % (storage, N, V, hw, cr, ld, accumulate)
    assert_within(dk, rk, 1e-5 * A_k, "dkernel " + what)
    assert_within(db, rb, 1e-5 * A_b, "dbias " + what)
    out = dd.cpu()
    base = dst.to(F64) if accumulate else torch.zeros(N * V, hw, cr, dtype=F64)
    exact = base + term.reshape(N * V, hw, cr)
    if eps is None:
        bound = 1e-6 * (base.abs() + term.reshape(N * V, hw, cr).abs())
    else:
        bound = eps * exact.abs() + tiny
    assert_within(out[:, :, :cr], exact, bound, "draw " + what)
    assert bool((out[:, :, cr:].to(F64) == SENT).all()) and bool((rd.cpu()[:, :, cr:].to(F64) == SENT).all())
    assert float(term.abs().max()) > 0


# ---- the engine -----------------------------------------------------------------------------------------------------
def _init(backbone, N, V, size, classes):
    p = TrainPlan(N * V, size, size, backbones.MATH_MODES["bf16x3"])
    taps = backbones.TAPS[backbone]
    if backbone == "inception_v3":
        backbones.build_inception_v3(p, keep=taps, fuse_siblings=True)
    else:
        backbones.build_resnet_v2_50(p, keep=taps)
    P = gparams.init_backbone_params(p.param_shapes(), seed=2, perturb_bn=True)
    H = gparams.init_head_params(V, p.end_points[taps[0]].c, p.end_points[taps[1]].c, classes, seed=3, spread_scores=True)
    return P, H


def _engine(backbone, N, V, size, train_scorer, storage="f32", init=None, **kw):
    P, H = init or _init(backbone, N, V, size, 5)
    return TrainGVCNN(backbone, N, V, size, size, 5, G, backbone_params=P, head_params=H, device=DEV, per_shape=True,
                      weight_mode="mean_score", storage=storage, train_scorer=train_scorer, **kw)


def _batch(N, V, size):
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    return x, torch.arange(N) % 5


def _pair(backbone, N, V, size, storage="f32"):
    """(option off, option on) on the same variables and batch, after one forward + backward; the forward outputs."""
    init = _init(backbone, N, V, size, 5)
    x, labels = _batch(N, V, size)
    engs, fwd = [], []
    for on in (False, True):
        eng = _engine(backbone, N, V, size, on, storage, init)
        scores, S, logits, loss = eng.forward(x, labels)
        fwd.append([t.clone() for t in (scores, S, logits, loss)])
        eng.backward()
        engs.append(eng)
    gi = engs[1].gidx_ps.cpu()
    # every shape has at least two non-empty groups: otherwise every gradient under test is 0
    assert all(len(set(gi[n].tolist())) >= 2 for n in range(N)), gi
    return engs[0], engs[1], fwd


def _reference(eng):
    """scorer_ref on the engine's own stored taps, dS, scorer and group indices."""
    N, V, r, f = eng.N, eng.V, eng.raw, eng.final
    raw = eng.view(r).cpu().to(F64).reshape(N, V, r.h * r.w, r.c)
    Fv = eng.view(f).cpu().to(F64).reshape(N, V, -1)
    dS = eng.dS.cpu().to(F64).reshape(N, -1)
    return R.head_chain(raw, Fv, dS, eng.score_kernel.cpu().to(F64), eng.score_bias.cpu().to(F64), eng.gidx_ps.cpu(), G,
                        "max")


def _scorer_grads(eng):
    ks, bs = zip(*(gparams.scorer_names(v) for v in range(eng.V)))
    return (torch.stack([eng.grads[k].reshape(-1) for k in ks]).cpu(), torch.cat([eng.grads[b] for b in bs]).cpu())


def _check_forward_and_scorer_grads(off, on, fwd, what):
    for a, b, name in zip(fwd[0], fwd[1], ("scores", "S", "logits", "loss")):
        assert torch.equal(a, b), name                          # (a) the option changes nothing in the forward pass
    ref = _reference(on)
    dk, db = _scorer_grads(on)
    assert_within(dk, ref["dkernel"], 1e-5 * ref["A_kernel"], "engine dkernel " + what)       # (c)
    assert_within(db, ref["dbias"], 1e-5 * ref["A_bias"], "engine dbias " + what)
    assert_within(on.dw_ps, ref["dw"], 1e-5 * ref["A_w"], "engine dw " + what)
    assert float(dk.abs().max()) > 0 and float(db.abs().max()) > 0                            # (e)
    first = [k for k in off.grads if k.endswith("/weights")][0]
    trunk = [k for k in off.grads if k.endswith("/weights") and ("block1" in k or "Conv2d_1a" in k or "Mixed_5" in k)]
    assert trunk, first
    assert any(not torch.equal(off.grads[k], on.grads[k]) for k in trunk)
    assert all(bool(torch.isfinite(g_).all()) for g_ in on.grads.values())
    return ref


def test_engine_resnet_fp32():
    """Test 3 of the issue on resnet_v2_50 64x64, N=3, V=4: (a) forward bitwise, (b) classifier and block4 gradients
    bitwise, (c) scorer gradients vs the reference, (d) the raw tap's gradient grows by exactly the injected term,
    (e) the gradient reaches block1."""
    N, V = 3, 4
    off, on, fwd = _pair("resnet_v2_50", N, V, 64)
    _check_forward_and_scorer_grads(off, on, fwd, "resnet f32")
    above = [k for k in off.grads if "/block4/" in k] + list(off.cls_names)                   # (b)
    assert len(above) > 10
    for k in above:
        assert torch.equal(off.grads[k], on.grads[k]), k
    for k in gparams.scorer_names(0):
        assert k in on.grads and k in on.momentum and k not in off.grads and k not in off.momentum
    # (d) the raw tap's gradient is read after a backward pass that keeps it in its own buffer (with the residual
    # aliasing of ResNet units the buffer goes on to hold the shortcut's gradient).  The injected term is what the
    # device's own dw_ps gives through the fp64 formulas: this checks the store-then-accumulate path, (c) the values.
    x, labels = _batch(N, V, 64)
    tap = []
    for eng in (off, on):
        eng.alias_residual_grad = False
        eng.forward(x, labels)
        eng.backward()
        tap.append(eng.view(eng.raw, grad=True).cpu().to(F64))
    r = on.raw
    dr, dr_abs = R.response_grad(on.r_img.cpu().to(F64).reshape(N, V), on.gidx_ps.cpu(), on.dw_ps.cpu().to(F64), G)
    raw = on.view(r).cpu().to(F64).reshape(N, V, r.h * r.w, r.c)
    term = R.scorer_grad(raw, on.score_kernel.cpu().to(F64), dr, dr_abs)[2].reshape(tap[0].shape)
    assert float(term.abs().max()) > 0
    assert_within(tap[1] - tap[0], term, 1e-6 * (tap[0].abs() + term.abs()), "raw-tap gradient, with - without")


def test_engine_inception_fp32():
    """(a), (c), (e) on inception_v3 139x139, N=2, V=3: the raw tap Mixed_6e is a concat output with several readers
    (two convolutions and a pool add to the stored scorer term)."""
    off, on, fwd = _pair("inception_v3", 2, 3, 139)
    _check_forward_and_scorer_grads(off, on, fwd, "inception f32")


def _state(eng):
    d = {("p", k): v for k, v in eng.params.items()}
    d.update({("m", k): v for k, v in eng.momentum.items()})
    d["score_kernel"], d["score_bias"] = eng.score_kernel, eng.score_bias
    return d


def test_engine_bf16_storage():
    """Test 4: forward bitwise equal to the option-off engine, scorer gradients within 2^-8 (norm-wise) of the reference
    on the engine's stored bf16 taps, finite loss, and train_step twice from the same state gives the same bits."""
    N, V = 3, 4
    off, on, fwd = _pair("resnet_v2_50", N, V, 64, "bf16")
    for a, b, name in zip(fwd[0], fwd[1], ("scores", "S", "logits", "loss")):
        assert torch.equal(a, b), name
    assert np.isfinite(float(fwd[1][3]))
    ref = _reference(on)
    dk, db = _scorer_grads(on)
    for dev, want, name in ((dk, ref["dkernel"], "dkernel"), (db, ref["dbias"], "dbias")):
        err, nrm = float((dev.to(F64) - want).norm()), float(want.norm())
        print("bf16 engine %s: |dev - ref| = %.3e, |ref| = %.3e" % (name, err, nrm))
        assert nrm > 0 and err <= 2.0 ** -8 * nrm, name
    x, labels = _batch(N, V, 64)
    snap = {k: v.clone() for k, v in _state(on).items()}
    runs = []
    for _ in range(2):
        for k, v in _state(on).items():
            v.copy_(snap[k])
        on._packed_dirty = True
        on.train_step(x, labels, lr=1e-2)
        on.train_step(x, labels, lr=1e-2)
        runs.append({k: v.clone() for k, v in _state(on).items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert not torch.equal(runs[0]["score_kernel"], snap["score_kernel"])


def test_five_steps_move_the_scorer_only_when_asked():
    """Test 5: five steps on a fixed batch change score_kernel / score_bias and fill their Momentum; with the option off
    the same steps leave the scorer bit for bit where it was (today's behaviour)."""
    N, V = 3, 4
    init = _init("resnet_v2_50", N, V, 64, 5)
    x, labels = _batch(N, V, 64)
    for train_scorer in (True, False):
        eng = _engine("resnet_v2_50", N, V, 64, train_scorer, init=init)
        k0, b0 = eng.score_kernel.clone(), eng.score_bias.clone()
        for _ in range(5):
            loss = eng.train_step(x, labels, lr=1e-2)
        assert np.isfinite(float(loss))
        if not train_scorer:
            assert torch.equal(eng.score_kernel, k0) and torch.equal(eng.score_bias, b0)
            continue
        assert not torch.equal(eng.score_kernel, k0) and not torch.equal(eng.score_bias, b0)
        assert tuple(eng.score_kernel.shape) == tuple(k0.shape) and tuple(eng.score_bias.shape) == tuple(b0.shape)
        for v in range(V):
            for name in gparams.scorer_names(v):
                m = eng.momentum[name]
                assert float(m.abs().max()) > 0 and bool(torch.isfinite(m).all()), name
        for t in list(eng.params.values()) + [eng.score_kernel, eng.score_bias]:
            assert bool(torch.isfinite(t).all())


def test_constructor_refusals():
    """Test 6 (the constructor needs the device, the refusals do not)."""
    kw = dict(device=DEV, train_scorer=True)
    with pytest.raises(ValueError, match="per_shape"):
        TrainGVCNN("resnet_v2_50", 2, 2, 64, 64, 5, G, weight_mode="mean_score", **kw)
    with pytest.raises(ValueError, match="mean_score"):
        TrainGVCNN("resnet_v2_50", 2, 2, 64, 64, 5, G, per_shape=True, weight_mode="count", **kw)
    with pytest.raises(ValueError, match="head_views"):
        TrainGVCNN("resnet_v2_50", 2, 2, 64, 64, 5, G, per_shape=True, weight_mode="mean_score", head_views=4, **kw)
    with pytest.raises(ValueError, match="view_offset"):
        TrainGVCNN("resnet_v2_50", 2, 2, 64, 64, 5, G, per_shape=True, weight_mode="mean_score", head_views=2,
                   view_offset=1, **kw)


def test_checkpoint_carries_the_scorer_slots(tmp_path):
    """Test 7: save after two steps, restore into a fresh engine (other initial values): variables, Momentum slots
    (scorer included) and global_step come back bit for bit and the next step is the same; an option-off engine's
    keys carry no Momentum for the scorer names."""
    N, V = 2, 3
    x, labels = _batch(N, V, 64)
    a = _engine("resnet_v2_50", N, V, 64, True)
    ta = Trainer(a, base_learning_rate=1e-2)
    ta.step(x, labels)
    ta.step(x, labels)
    prefix = str(tmp_path / "scorer.ckpt")
    ta.save(prefix)
    scorer = [n for v in range(V) for n in gparams.scorer_names(v)]
    sd = ta.state_dict()
    for n in scorer:
        assert n in sd and n + "/Momentum" in sd and sd[n + "/Momentum"].shape == sd[n].shape, n
        assert float(np.abs(sd[n + "/Momentum"]).max()) > 0, n
    b = TrainGVCNN("resnet_v2_50", N, V, 64, 64, 5, G, device=DEV, per_shape=True, weight_mode="mean_score",
                   train_scorer=True, seed=7)
    assert not torch.equal(a.score_kernel, b.score_kernel)
    tb = Trainer(b, base_learning_rate=1e-2)
    assert tb.restore(prefix, strict=True) == []
    assert tb.global_step == ta.global_step == 2
    sa, sb = _state(a), _state(b)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    la, lb = ta.step(x, labels).clone(), tb.step(x, labels).clone()
    assert torch.equal(la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    off = _engine("resnet_v2_50", N, V, 64, False)
    keys = set(Trainer(off).state_dict())
    assert not any(n + "/Momentum" in keys for n in scorer) and all(n in keys for n in scorer)
    trainable = [k for k in off.params if not k.endswith(("moving_mean", "moving_variance"))]
    assert {k for k in keys if k.endswith("/Momentum")} == {k + "/Momentum" for k in trainable}
