"""CPU checks of the logit attribution: the fp64 reference (tests/explain_ref.py) against autograd, the argument checks
of gv_explain_views through the C ABI (no launch, no GPU), and the overlay blend of tools/explain_views.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import explain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(per_shape, seed):
    """Integer-valued F (ties are frequent), a view in two groups, an empty group."""
    rng = np.random.RandomState(seed)
    N, V, hw, C, G, nc = 3, 6, 4, 7, 5, 4
    F = rng.randint(-2, 3, size=(N, V, hw, C)).astype(np.float64)
    K = rng.randn(C, nc)
    b = rng.randn(nc)

    def scheme():
        s = np.zeros((G, V), dtype=np.int32)
        for v in range(V):
            s[rng.randint(0, G - 1), v] = 1          # group G-1 stays empty
        s[(np.argmax(s[:, 0]) + 1) % (G - 1), 0] = 1  # view 0 sits in two groups
        return s
    if per_shape:
        sch = np.stack([scheme() for _ in range(N)])
        w = rng.rand(N, G) + 0.5
    else:
        sch = scheme()
        w = 1.0 + sch.sum(1).astype(np.float64)
    return F, sch, w, K, b, rng.randint(0, nc, size=N)


def _torch_logits(F, sch, w, K, b, pool, fill):
    N, V, hw, C = F.shape
    rows = []
    for n in range(N):
        s, wt = (sch[n], w[n]) if sch.ndim == 3 else (sch, w)
        S = 0
        for g in range(s.shape[0]):
            idx = np.nonzero(s[g])[0].tolist()
            if not idx:
                D = torch.full((hw, C), fill, dtype=torch.float64)
            else:
                D = torch.amax(F[n, idx], dim=0) if pool == "max" else torch.mean(F[n, idx], dim=0)
            S = S + float(wt[g]) * D
        S = S / float(np.sum(wt))
        rows.append(S.mean(0) @ torch.from_numpy(K) + torch.from_numpy(b))
    return torch.stack(rows)


@pytest.mark.parametrize("per_shape", [False, True])
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_reference_matches_autograd_and_is_complete(pool, per_shape):
    F, sch, w, K, b, tg = _case(per_shape, 3 + per_shape)
    fill = 1.0
    Ft = torch.from_numpy(F).requires_grad_(True)
    logits = _torch_logits(Ft, sch, w, K, b, pool, fill)        # torch.amax splits a tied maximum equally
    picked = logits[torch.arange(F.shape[0]), torch.from_numpy(tg)]
    (g_auto,) = torch.autograd.grad(picked.sum(), Ft)
    g_ref, _, ng = ref.gradient(F, sch, w, K, tg, pool)
    assert ng.max() == 2 and ng.min() == 1
    np.testing.assert_allclose(g_ref, g_auto.numpy(), rtol=0, atol=1e-12)
    fwd = ref.forward_logits(F, sch, w, K, b, pool, fill)
    np.testing.assert_allclose(fwd, logits.detach().numpy(), rtol=0, atol=1e-12)
    out = ref.explain(F, sch, w, K, b, tg, pool, fill, "exact")
    total = out["baseline"][0] + out["maps"][0].sum((1, 2))
    np.testing.assert_allclose(total, fwd[np.arange(F.shape[0]), tg], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["view_contrib"][0], out["maps"][0].sum(2), rtol=0, atol=1e-12)
    cam = ref.explain(F, sch, w, K, b, tg, pool, fill, "gradcam")
    np.testing.assert_allclose(cam["alpha"][0], g_ref.mean(2), rtol=0, atol=1e-12)
    assert (cam["maps"][0] >= 0).all()
    np.testing.assert_array_equal(cam["view_contrib"][0], out["view_contrib"][0])


def test_reference_zero_weight_shape():
    F, sch, w, K, b, tg = _case(True, 5)
    w[1] = 0.0
    out = ref.explain(F, sch, w, K, b, tg, "max", 1.0, "exact")
    assert not out["maps"][0][1].any() and out["baseline"][0][1] == b[tg[1]]
    assert ref.forward_logits(F, sch, w, K, b)[1, tg[1]] == b[tg[1]]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


def test_explain_argument_checks(lib):
    """Every refusal comes before any launch, so fake non-null pointers (16) are enough."""
    P = 16
    ok = dict(F=P, V=6, N=2, hw=4, C=64, vs=256, ss=1536, scheme=P, G=5, weight=P, per_shape=0, pool=0, fill=1.0, K=P,
              b=P, nc=10, logits=P, targets=None, kind=0, maps=P, contrib=P, baseline=P, target_out=P, status=P, ws=None,
              dtype=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gv_explain_views(*[a[k] for k in ok])
    BAD, UNS = -1, -2
    for name in ("F", "scheme", "weight", "K", "b", "maps", "contrib", "baseline", "target_out", "status"):
        assert call(**{name: None}) == BAD, name
    assert call(logits=None, targets=None) == BAD              # nothing to take the class from
    for name in ("V", "N", "hw", "C", "G", "nc"):
        assert call(**{name: 0}) == BAD, name
    assert call(vs=-1) == BAD and call(ss=-1) == BAD
    assert call(V=65) == UNS and call(G=65) == UNS and call(N=65536) == UNS
    assert call(kind=9) == BAD
    assert call(pool=9) == BAD
    assert call(kind=1, ws=None) == BAD                        # gradcam without its workspace
    assert call(dtype=7) == UNS
    # alpha [N, V, C] and the per-chunk shares of view_contrib [N, V, ceil(C / 64)], fp32; nothing for 'exact'
    assert lib.gv_explain_workspace_bytes(6, 2, 64, 0) == 0
    assert lib.gv_explain_workspace_bytes(6, 2, 64, 1) == 4 * 2 * 6 * (64 + 1)
    assert lib.gv_explain_workspace_bytes(12, 32, 2048, 1) == 4 * 32 * 12 * (2048 + 32)
    assert lib.gv_explain_workspace_bytes(5, 2, 20, 1) == 4 * 2 * 5 * (20 + 1)
    assert lib.gv_explain_workspace_bytes(0, 2, 64, 1) == BAD
    assert lib.gv_explain_workspace_bytes(6, 2, 64, 9) == BAD


def test_overlay_blend():
    spec = importlib.util.spec_from_file_location("explain_views_tool", os.path.join(ROOT, "tools", "explain_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    views = np.full((2, 2, 2, 3), 100, dtype=np.uint8)
    maps = np.array([[[2.0, -1.0], [0.0, 0.5]], [[0.0, 0.0], [-2.0, 0.0]]])
    out = tool.blend(views, maps, strength=0.5)
    assert out.shape == (2, 4, 3) and out.dtype == np.uint8
    # mix a = 0.5 * |m| / 2: red for m > 0, blue for m < 0, untouched at 0; views side by side
    assert out[0, 0].tolist() == [178, 50, 50]                 # m = 2: a = 0.5 -> 50 + 127.5 -> rint(177.5) = 178
    assert out[0, 1].tolist() == [75, 75, 139]                 # m = -1: a = 0.25 -> 75, 75 + 63.75
    assert out[1, 0].tolist() == [100, 100, 100]
    assert out[1, 1].tolist() == [119, 88, 88]                 # m = 0.5: a = 0.125 -> 87.5 + 31.875, 87.5 -> 88
    assert out[1, 2].tolist() == [50, 50, 178]                 # second view, m = -2
    assert out[0, 2].tolist() == [100, 100, 100]
    flat = tool.blend(views, np.zeros((2, 2, 2)))
    assert (flat == 100).all()
