"""Argument codes of the scorer-gradient entry points (csrc/scorer_bwd.hip) and the refusals around them.  Every call in
the tables is rejected before any HIP call, so this runs without a device; the codes are literals.  Also: the closed
forms the kernels implement against the autograd reference of tests/scorer_ref.py (fp64, CPU)."""
import os
import types

import pytest
import torch                                       # noqa: F401  (before the library, as in the GPU test files)

from gvcnn_tf_amd import _lib

import scorer_ref as R                             # noqa: E402

P = 4096                                           # a 16-byte aligned stand-in address: never dereferenced
F32, BF16, F16 = _lib.GV_F32, _lib.GV_BF16, _lib.GV_F16
BADARG, UNSUPPORTED, ALIGN = -1, -2, -3

# N=2, E=100 -> one chunk of 256 scalars per shape: 2 * 1 * 3 * 4 bytes
GW = dict(F=P, dS=P, V=4, N=2, E=100, vs=100, ss=400, scheme=P, G=3, weight=P, mode=0, dw=P, ws=P, ws_bytes=24)
SB = dict(raw=P, nb=6, hw=4, cr=8, raw_ld=8, kernel=P, r_img=P, gidx=P, dw=P, G=3, V=3, dkernel=P, dbias=P, draw=P,
          draw_ld=8, accumulate=0)


def nulls(*names):
    return [({n: None}, BADARG) for n in names]


CASES = {
    "gv_group_weight_bwd_per_shape": (GW, nulls("F", "dS", "scheme", "weight", "dw", "ws") + [
        (dict(V=0), BADARG), (dict(N=0), BADARG), (dict(E=0), BADARG), (dict(G=0), BADARG), (dict(vs=-1), BADARG),
        (dict(mode=2), BADARG), (dict(ws_bytes=23), BADARG), (dict(ws_bytes=0), BADARG),
        (dict(E=257, vs=257, ss=4 * 257), BADARG),                       # two chunks now: 24 bytes are short
        (dict(V=65), UNSUPPORTED), (dict(G=65, ws_bytes=1 << 20), UNSUPPORTED), (dict(N=65536, ws_bytes=1 << 24), UNSUPPORTED),
        (dict(V=65, F=None), BADARG), (dict(ws=P + 2), ALIGN)]),
    "gv_view_score_bwd": (SB, nulls("raw", "kernel", "r_img", "gidx", "dw", "dkernel", "dbias") + [
        (dict(nb=0), BADARG), (dict(hw=0), BADARG), (dict(cr=0), BADARG), (dict(raw_ld=7), BADARG),
        (dict(draw_ld=7), BADARG), (dict(G=0), BADARG), (dict(V=0), BADARG), (dict(nb=7), BADARG),
        (dict(accumulate=2), BADARG), (dict(V=65, nb=130), UNSUPPORTED), (dict(G=65), UNSUPPORTED),
        (dict(nb=65538, V=2), UNSUPPORTED), (dict(V=65, nb=130, raw=None), BADARG)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_scorer_entry_point_argument_codes(name):
    lib = _lib.load()
    base, cases = CASES[name]
    fn = getattr(lib, name)
    for change, code in cases:
        assert set(change) <= set(base), change
        for dtype in (F32, BF16, F16):
            a = dict(base)
            a.update(change)
            assert fn(*(list(a.values()) + [dtype, None])) == code, (name, change, dtype)
    for dtype in (3, -1, 255, 0x100 | BF16):       # an unknown dtype, whatever else is wrong
        assert fn(*(list(base.values()) + [dtype, None])) == UNSUPPORTED, (name, dtype)
        a = dict(base)
        a[next(iter(a))] = None
        assert fn(*(list(a.values()) + [dtype, None])) == UNSUPPORTED, (name, dtype)


def test_workspace_size_query():
    lib = _lib.load()
    q = lib.gv_group_weight_bwd_workspace_bytes
    assert q(2, 100, 3) == 24
    assert q(4, 5000, 10) == 4 * 20 * 10 * 4        # ceil(5000 / 256) = 20 chunks on the scalar path: every path fits
    assert q(0, 100, 3) == BADARG and q(2, 0, 3) == BADARG and q(2, 100, 0) == BADARG
    assert q(2, 100, 65) == UNSUPPORTED and q(65536, 100, 3) == UNSUPPORTED


def test_header_exports_and_signatures_name_the_entry_points():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gvcnn_hip.h")).read()
    for name in ("gv_group_weight_bwd_workspace_bytes", "gv_group_weight_bwd_per_shape", "gv_view_score_bwd"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["gv_group_weight_bwd_per_shape"][1]) == 16
    assert len(_lib.SIGNATURES["gv_view_score_bwd"][1]) == 18
    assert lib.gv_abi_version() == 1


def test_sharded_engine_refuses_a_scorer_training_engine():
    from gvcnn_tf_amd import sharding
    eng = types.SimpleNamespace(train_scorer=True, per_shape=True, N=2, V=2, Vh=2)
    with pytest.raises(ValueError, match="train_scorer"):
        sharding.ShardedTrainGVCNN(eng, mode="not a mode")               # refused before any other check


def test_reference_autograd_equals_the_closed_forms():
    """(A self-check of the reference, not of the product: it uses no product code and passes without the feature.)
    scorer_ref's autograd against the formulas the kernels implement, written out: dw = (1/W) sum dS (D_g - S),
    ds = dw / |M|, dr = ds sign(r) (1 - s)^2, dbias = sum_n dr, dkernel = sum_n dr mean_p raw, draw = dr k / hw."""
    g = torch.Generator().manual_seed(0)
    N, V, G, E, hw, cr = 3, 5, 10, 96, 4, 24
    for pool in ("max", "mean"):
        raw = torch.randn(N, V, hw, cr, generator=g, dtype=torch.float64)
        Fv = torch.randn(N, V, E, generator=g, dtype=torch.float64)
        dS = torch.randn(N, E, generator=g, dtype=torch.float64)
        k = torch.randn(V, cr, generator=g, dtype=torch.float64) * 0.3
        b = torch.randn(V, generator=g, dtype=torch.float64)
        r = (raw.mean(2) * k[None]).sum(-1) + b[None]
        s = R.score_of(r)
        gidx = (s * 10).to(torch.int64)
        gidx[2, 1] = 11                                                   # a view in no group
        out = R.head_chain(raw, Fv, dS, k, b, gidx, G, pool)
        mask, cnt = R.members(gidx, G)
        w = R.mean_score_weights(s, mask, cnt)
        D = R.pooled(Fv, mask, pool)
        S, W = R.fuse(D, w, cnt)
        dw = (dS[:, None, :] * (D - S[:, None, :])).sum(-1) / W[:, None] * (cnt > 0)
        assert len(set(gidx[0].tolist())) > 1 and float(dw.abs().max()) > 0
        dr = torch.zeros(N, V, dtype=torch.float64)
        for n in range(N):
            for v in range(V):
                gi = int(gidx[n, v])
                if 0 <= gi < G:
                    dr[n, v] = dw[n, gi] / cnt[n, gi] * torch.sign(r[n, v]) * (1 - s[n, v]) ** 2
        assert float(dr[2, 1]) == 0.0
        ref = {"dw": dw, "dbias": dr.sum(0), "dkernel": (dr[:, :, None] * raw.mean(2)).sum(0),
               "draw": (dr[:, :, None, None] * k[None, :, None, :] / hw).expand(N, V, hw, cr)}
        for key, want in ref.items():
            err = float((out[key] - want).abs().max())
            assert err <= 1e-12 * max(1.0, float(want.abs().max())), (pool, key, err)
        assert bool((out["dkernel"].abs() <= out["A_kernel"] * (1 + 1e-9)).all())
        assert bool((out["dbias"].abs() <= out["A_bias"] * (1 + 1e-9)).all())
