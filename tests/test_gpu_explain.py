"""GPU tests of the logit attribution (csrc/explain.hip, GVCNN.explain) against the fp64 restatement in
tests/explain_ref.py: integer fixtures bit for bit, real-valued data within a bound derived from the reference's own term
counts, the project's backward pass as a second witness, the whole path through the engines, determinism, meshes.

Bound of the real-valued cases: an fp32 sum of n terms whose absolute values add up to T, each term made with at most 8
roundings, is within (n + 8) * 2^-24 * T of the exact value (first order; the 1.01 absorbs the higher orders)."""
import numpy as np
import pytest
import torch

import gvcnn_tf_amd as gv
from gvcnn_tf_amd import _lib, model

import explain_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
TYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
KINDS = ("exact", "gradcam")


def host(t):
    t = t.detach().cpu()
    return (t.to(torch.float32) if t.dtype in (torch.bfloat16, torch.float16) else t).numpy()     # lossless


def stored(F, ty):
    """(device tensor in the storage type, the same values as fp64 on the host)"""
    Fd = torch.from_numpy(np.asarray(F, np.float32)).to(DEV).to(TYPES[ty]).contiguous()
    return Fd, host(Fd.to(torch.float64))


def check_bound(name, got, triple, worst):
    val, n, T = triple
    err = np.abs(got.astype(np.float64) - val)
    bound = 1.01 * (n + 8) * U * T
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert (err <= bound).all(), "%s: error / bound = %.3f" % (name, ratio)


# ---- 1. integer fixtures: every quantity is a dyadic rational with few bits, no summation order can change it -------
def fixture(pool, C, seed=0):
    rng = np.random.RandomState(seed + C)
    N, V, G, h, w, nc = 3, 6, 5, 2, 2, 4
    F = rng.randint(-3, 4, size=(N, V, h, w, C)).astype(np.float64)
    K = rng.randint(-2, 3, size=(C, nc)).astype(np.float64)
    b = rng.randint(-3, 4, size=nc).astype(np.float64)
    scheme = np.zeros((G, V), dtype=np.int32)
    groups = [[0, 1], [2, 3], [4], [5, 0], []] if pool == "max" else [[0], [1, 2], [2, 3, 4, 5], [0, 5], []]
    for g, members in enumerate(groups):
        scheme[g, members] = 1
    weight = np.array([2, 2, 1, 2, 1], dtype=np.float64)        # sums to 8; the empty group keeps weight 1, fill 1.0
    return F, scheme, weight, K, b, np.array([0, 2, 1])


@pytest.mark.parametrize("ty", list(TYPES))
@pytest.mark.parametrize("C", [20, 64])                          # scalar path / 16-byte path
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_integer_fixtures_bit_for_bit(pool, C, ty):
    F, scheme, weight, K, b, tg = fixture(pool, C)
    Fd, Fs = stored(F, ty)
    assert (Fs == F).all()
    N, V, h, w, _ = F.shape
    sch = torch.from_numpy(scheme).to(DEV)
    wt = torch.from_numpy(weight.astype(np.float32)).to(DEV)
    Kd = torch.from_numpy(K.astype(np.float32)).to(DEV)
    bd = torch.from_numpy(b.astype(np.float32)).to(DEV)
    for kind in KINDS:
        want = ref.explain(Fs.reshape(N, V, h * w, C), scheme, weight, K, b, tg, pool, 1.0, kind)
        ex = gv.explain_views(Fd, sch, wt, Kd, bd, target=tg, pool=pool, empty_fill=1.0, kind=kind)
        assert host(ex.target).tolist() == tg.tolist()
        assert (host(ex.maps).reshape(N, V, h * w).astype(np.float64) == want["maps"][0]).all(), kind
        assert (host(ex.view_contrib).astype(np.float64) == want["view_contrib"][0]).all(), kind
        assert (host(ex.baseline).astype(np.float64) == want["baseline"][0]).all(), kind
        assert np.abs(want["maps"][0]).max() > 0 and (want["baseline"][0] != b[tg]).any()
    E = h * w * C
    out = model._explain_launch(Fd.data_ptr(), model._STORAGE_OF[Fd.dtype], N, V, h, w, C, E, V * E, sch, wt, False, pool,
                                1.0, Kd, bd, None, torch.from_numpy(tg).to(DEV), "gradcam", True, DEV)
    alpha = host(out[4])[:N * V * C].reshape(N, V, C)
    assert (alpha.astype(np.float64) == want["alpha"][0]).all()


# ---- 2. real-valued cases within the derived bound ---------------------------------------------------------------
def real_case(name, seed=1):
    rng = np.random.RandomState(seed)
    nc = 7
    if name == "two_groups":
        N, V, hw, C, G = 2, 5, 9, 20, 4
    elif name == "wide":
        N, V, hw, C, G = 2, 12, 25, 256, 10
    elif name == "v64":
        N, V, hw, C, G = 1, 64, 1, 8, 64
    else:
        N, V, hw, C, G = 3, 6, 4, 64, 5
    F = np.maximum(rng.randn(N, V, hw, C), 0.0)                  # about half the entries exact zeros: ties at zero
    K, b = rng.randn(C, nc), rng.randn(nc)

    def one_hot():
        s = np.zeros((G, V), dtype=np.int32)
        s[rng.randint(0, G, size=V), np.arange(V)] = 1
        return s
    if name == "per_shape":
        scheme = np.stack([one_hot() for _ in range(N)])
        weight = rng.rand(N, G).astype(np.float32)
        weight[1] = 0.0                                          # sum w = 0: S = 0 for that shape
    else:
        scheme = one_hot()
        if name == "two_groups":
            scheme[(int(np.argmax(scheme[:, 1])) + 1) % G, 1] = 1
        weight = (1 + scheme.sum(1)).astype(np.float32)
    return F, scheme, weight, K.astype(np.float32), b.astype(np.float32), rng.randint(0, nc, size=N)


_REAL = {}


def real(name):
    if name not in _REAL:
        _REAL[name] = real_case(name)
    return _REAL[name]


@pytest.mark.parametrize("ty", list(TYPES))
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("name", ["two_groups", "wide", "v64", "per_shape"])
def test_real_values_within_bound(name, pool, ty, capsys):
    F, scheme, weight, K, b, tg = real(name)
    N, V, hw, C = F.shape
    Fd, Fs = stored(F.reshape(N, V, 1, hw, C), ty)
    Fs = Fs.reshape(N, V, hw, C)
    sch, wt = torch.from_numpy(scheme).to(DEV), torch.from_numpy(weight).to(DEV)
    Kd, bd = torch.from_numpy(K).to(DEV), torch.from_numpy(b).to(DEV)
    logits = ref.forward_logits(Fs, scheme, weight, K, b, pool, 1.0).astype(np.float32)
    arg = np.argmax(logits, axis=1)                              # the first maximum
    worst = {}
    for kind in KINDS:
        for targets, kw in ((tg, dict(target=tg)), (arg, dict(logits=torch.from_numpy(logits).to(DEV)))):
            want = ref.explain(Fs, scheme, weight, K, b, targets, pool, 1.0, kind)
            ex = gv.explain_views(Fd, sch, wt, Kd, bd, pool=pool, empty_fill=1.0, kind=kind, **kw)
            assert host(ex.target).tolist() == targets.tolist()
            check_bound(kind + " maps", host(ex.maps).reshape(N, V, hw), want["maps"], worst)
            check_bound(kind + " view_contrib", host(ex.view_contrib), want["view_contrib"], worst)
            check_bound(kind + " baseline", host(ex.baseline), want["baseline"], worst)
            if name == "per_shape":
                assert not host(ex.maps)[1].any() and not host(ex.view_contrib)[1].any()
                assert host(ex.baseline)[1] == b[targets[1]]
    with capsys.disabled():
        print("\n  %s %s %s: largest error / bound %s" % (name, pool, ty, {k: round(v, 4) for k, v in worst.items()}))


def test_target_out_of_range():
    F, scheme, weight, K, b, tg = real("two_groups")
    N, V, hw, C = F.shape
    Fd, _ = stored(F.reshape(N, V, 1, hw, C), "f32")
    args = (Fd, torch.from_numpy(scheme).to(DEV), torch.from_numpy(weight).to(DEV), torch.from_numpy(K).to(DEV),
            torch.from_numpy(b).to(DEV))
    bad = np.array([tg[0], K.shape[1]])
    for kind in KINDS:
        with pytest.raises(IndexError):
            gv.explain_views(*args, target=bad, kind=kind)
        ex = gv.explain_views(*args, target=bad, kind=kind, check=False)
        good = gv.explain_views(*args, target=tg, kind=kind)
        assert host(ex.target).tolist() == [tg[0], -1]
        assert not host(ex.maps)[1].any() and not host(ex.view_contrib)[1].any() and host(ex.baseline)[1] == 0
        assert host(ex.maps)[0].tobytes() == host(good.maps)[0].tobytes()
    with pytest.raises(ValueError):
        gv.explain_views(*args)                                   # neither logits nor a target


# ---- 3. the project's own backward as a second witness -------------------------------------------------------------
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("name", ["two_groups", "wide", "per_shape"])
def test_against_view_pool_fuse_backward(name, pool):
    F, scheme, weight, K, b, tg = real(name)
    N, V, hw, C = F.shape
    Fd, Fs = stored(F.reshape(N, V, 1, hw, C), "f32")
    Fs = Fs.reshape(N, V, hw, C)
    sch, wt = torch.from_numpy(scheme).to(DEV), torch.from_numpy(weight).to(DEV)
    dS = np.stack([np.broadcast_to(K[:, tg[n]] / np.float32(hw), (hw, C)) for n in range(N)]).astype(np.float32)
    dSd = torch.from_numpy(np.ascontiguousarray(dS)).to(DEV)
    dF = torch.zeros_like(Fd)
    E = hw * C
    lib = _lib.load()
    fn = lib.gv_view_pool_fuse_bwd_per_shape if scheme.ndim == 3 else lib.gv_view_pool_fuse_bwd
    G = scheme.shape[-2]
    _lib.check(fn(Fd.data_ptr(), dSd.data_ptr(), V, N, E, E, V * E, sch.data_ptr(), G, wt.data_ptr(),
                  0 if pool == "max" else 1, dF.data_ptr(), None), "gv_view_pool_fuse_bwd")
    via_bwd = (Fs * host(dF).reshape(N, V, hw, C).astype(np.float64)).sum(3)
    want = ref.explain(Fs, scheme, weight, K, b, tg, pool, 1.0, "exact")
    ex = gv.explain_views(Fd, sch, wt, torch.from_numpy(K).to(DEV), torch.from_numpy(b).to(DEV), target=tg, pool=pool)
    _, n, T = want["maps"]
    err = np.abs(host(ex.maps).reshape(N, V, hw).astype(np.float64) - via_bwd)
    assert (err <= 1.01 * (n + 8) * U * T).all()
    assert np.abs(via_bwd).max() > 0


# ---- 4. the whole path ------------------------------------------------------------------------------------------------
def make_engine(backbone, size, storage, per_shape):
    N, V, C_, G = 2, 6, 10, 10
    kw = dict(per_shape=True, weight_mode="mean_score") if per_shape else {}
    eng = gv.GVCNN(backbone, N, V, size, size, C_, G, device=DEV, storage=storage, **kw)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    eng.plan.bind(P)
    eng.set_head(Hd)
    return eng


@pytest.mark.parametrize("per_shape", [False, True])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("backbone,size", [("resnet_v2_50", 64), ("inception_v3", 75)])
def test_engine_explain(backbone, size, storage, per_shape, capsys):
    eng = make_engine(backbone, size, storage, per_shape)
    N, V = eng.N, eng.V
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    before = [host(t).copy() for t in eng.forward(x)]
    F_before = host(eng.final_view_descriptors().to(torch.float32)).copy()
    ex = eng.explain(x)
    cam = eng.explain(x, kind="gradcam")
    state = [host(t).copy() for t in ((eng.scores_ps if per_shape else eng.scores), eng.shape_descriptor, eng.logits)]
    after = [host(t).copy() for t in eng.forward(x)]
    for a, s, c in zip(before, state, after):                    # explain leaves the engine as forward left it
        assert a.tobytes() == s.tobytes() == c.tobytes()
    assert host(ex.logits).tobytes() == before[2].tobytes() == host(cam.logits).tobytes()
    assert host(eng.final_view_descriptors().to(torch.float32)).tobytes() == F_before.tobytes()
    logits = before[2]
    k = np.argmax(logits, axis=1)
    assert host(ex.target).tolist() == k.tolist() == host(cam.target).tolist()
    f = eng.final
    hw, C = f.h * f.w, f.c
    assert tuple(ex.maps.shape) == (N, V, f.h, f.w) and tuple(ex.view_contrib.shape) == (N, V)
    scheme = host(eng.scheme_ps if per_shape else eng.scheme)
    weight = host(eng.weight_ps if per_shape else eng.weight)
    assert host(ex.weight).tobytes() == weight.tobytes()
    assert host(ex.gidx).tobytes() == host(eng.gidx_ps if per_shape else eng.gidx).tobytes()
    assert host(ex.scores).tobytes() == state[0].tobytes()
    Fs = F_before.astype(np.float64).reshape(N, V, hw, C)
    K, b = host(eng.cls_kernel), host(eng.cls_bias)
    want = ref.explain(Fs, scheme, weight, K, b, k, eng.pool, eng.empty_fill, "exact")
    maps = host(ex.maps).reshape(N, V, hw).astype(np.float64)
    worst = {}
    check_bound("maps", host(ex.maps).reshape(N, V, hw), want["maps"], worst)
    check_bound("view_contrib", host(ex.view_contrib), want["view_contrib"], worst)
    _, n_vc, T_vc = want["view_contrib"]
    assert (np.abs(host(ex.view_contrib) - maps.sum(2)) <= 1.01 * (n_vc + 8) * U * T_vc).all()
    # completeness: the forward rounds S to the storage type before the average pool (u), and both sides sum n terms
    u = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[storage]
    n_all = want["view_contrib"][1].sum(1) + want["baseline"][1]
    T_all = want["view_contrib"][2].sum(1) + want["baseline"][2]
    total = host(ex.baseline).astype(np.float64) + maps.sum((1, 2))
    gap = np.abs(logits[np.arange(N), k].astype(np.float64) - total)
    bound = (2.02 * (n_all + 8) * U + u) * T_all
    with capsys.disabled():
        print("\n  %s %s per_shape=%s: completeness error / bound %.4f, maps %.4f, view_contrib %.4f"
              % (backbone, storage, per_shape, float((gap / bound).max()), worst["maps"], worst["view_contrib"]))
    assert (gap <= bound).all()
    assert np.abs(maps).max() > 0
    assert (host(cam.maps) >= 0).all() and host(cam.maps).max() > 0
    check_bound("gradcam view_contrib", host(cam.view_contrib), want["view_contrib"], worst)
    assert tuple(ex.resized(size, size).shape) == (N, V, size, size)
    other = eng.explain(x, target=[1, 0])
    assert host(other.target).tolist() == [1, 0]
    with pytest.raises(IndexError):
        eng.explain(x, target=10)


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_same_bits(kind):
    F, scheme, weight, K, b, tg = real("wide")
    N, V, hw, C = F.shape
    Fd, _ = stored(F.reshape(N, V, 5, 5, C), "bf16")
    args = (Fd, torch.from_numpy(scheme).to(DEV), torch.from_numpy(weight).to(DEV), torch.from_numpy(K).to(DEV),
            torch.from_numpy(b).to(DEV))
    a = gv.explain_views(*args, target=tg, kind=kind)
    c = gv.explain_views(*args, target=tg, kind=kind)
    for name in ("target", "baseline", "view_contrib", "maps"):
        assert host(getattr(a, name)).tobytes() == host(getattr(c, name)).tobytes(), name


# ---- 6. meshes in -----------------------------------------------------------------------------------------------------
def test_explain_meshes_equals_explain_on_renders():
    from gvcnn_tf_amd import render as R
    eng = make_engine("resnet_v2_50", 64, "bf16", False)
    batch = R.MeshBatch([R.icosphere(1), R.icosphere(2)], DEV)
    r = R.ViewRenderer(eng.V, 64, 64, device=DEV)
    got = eng.explain_meshes(batch, renderer=r, kind="exact")
    want = eng.explain(r.render(batch), kind="exact")
    for name in ("logits", "target", "baseline", "view_contrib", "maps", "scores", "gidx", "weight"):
        assert host(getattr(got, name)).tobytes() == host(getattr(want, name)).tobytes(), name
