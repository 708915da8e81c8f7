"""Training step on 16-bit storage (BASELINE configs[2]: bf16 forward + backward; csrc/bn_train.hip, csrc/wgrad_lp.hip,
csrc/train.hip).

Every storage-typed kernel is checked against torch autograd through the CPU oracle's ops ON THE SAME 16-bit
representable inputs, so the only differences are the summation order (filter gradient, statistics) and the single
rounding of each stored output (tolerance 2^-8 relative for bf16 outputs, 2^-11 for fp16).  The whole step is then
held against the fp32 engine (itself pinned to the oracle in test_gpu_train.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import _lib                       # noqa: E402
from gvcnn_tf_amd.training import TrainGVCNN        # noqa: E402
from oracle import backbone as OB                   # noqa: E402
import bn_ref                                       # noqa: E402   (tests/bn_ref.py)
from slab import NAN, SENTINEL, _Slab, _hold        # noqa: E402   (tests/slab.py)

DEV = "cuda:0"
TYPES = [(_lib.GV_BF16, torch.bfloat16, 2.0 ** -8), (_lib.GV_F16, torch.float16, 2.0 ** -11)]


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def close(a, d, tol):
    a, d = np.asarray(a, dtype=np.float64), np.asarray(d, dtype=np.float64)
    scale = max(float(np.abs(d).max()), 1e-30)
    err = float(np.abs(a - d).max())
    assert err <= tol * scale, "max|diff| %.3e vs scale %.3e (%.2e rel)" % (err, scale, err / scale)


def q(t, tdt):
    """fp32 tensor with values representable in the storage type."""
    return t.to(tdt).to(torch.float32)


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("c,ld", [(32, 32), (40, 48), (12, 12)])
def test_bn_train_forward_and_backward_typed(dt, tdt, eps, c, ld):
    g = torch.Generator().manual_seed(0)
    N, V, h, w = 3, 4, 5, 6
    z = q(torch.randn(N * V, h, w, c, generator=g) * 2 + 0.5, tdt)
    beta, gamma = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    dy = q(torch.randn(N * V, h, w, c, generator=g), tdt)
    groups = [b % V for b in range(N * V)]

    def dev(t):                                         # [.., c] -> device tensor with pixel stride ld
        buf = torch.zeros(*t.shape[:-1], ld, dtype=tdt, device=DEV)
        buf[..., :c] = t.to(tdt).to(DEV)
        return buf

    for gm in (None, gamma):
        zz = z.clone().requires_grad_(True)
        be = beta.clone().requires_grad_(True)
        ga = gm.clone().requires_grad_(True) if gm is not None else None
        y_ref, mean_ref, var_ref = OB.batch_norm_train_grouped(zz, be, ga, 1e-3, groups)
        y_ref = torch.relu(y_ref)
        zd = dev(z)
        counts = torch.full((V,), N * h * w, dtype=torch.int32, device=DEV)
        accum = torch.zeros(2 * V * c, dtype=torch.float64, device=DEV)
        stt = {k: torch.empty(V, c, device=DEV) for k in ("mean", "var", "inv", "scale", "shift")}
        bd, gd = beta.to(DEV), (gm.to(DEV) if gm is not None else None)
        _lib.check(lib().gv_bn_sums_grouped_t(zd.data_ptr(), N * V, h * w, c, ld, V, accum.data_ptr(), dt, st()), "sums")
        _lib.check(lib().gv_bn_finalize_grouped(accum.data_ptr(), c, V, counts.data_ptr(),
                                                gd.data_ptr() if gd is not None else None, bd.data_ptr(), 1e-3,
                                                stt["mean"].data_ptr(), stt["var"].data_ptr(), stt["inv"].data_ptr(),
                                                stt["scale"].data_ptr(), stt["shift"].data_ptr(), st()), "finalize")
        yd = torch.zeros_like(zd)
        _lib.check(lib().gv_scale_shift_act_grouped_t(zd.data_ptr(), N * V, h * w, c, ld, stt["scale"].data_ptr(),
                                                      stt["shift"].data_ptr(), V, 1, yd.data_ptr(), ld, dt, st()),
                   "apply")
        close(stt["mean"].cpu(), mean_ref.detach(), 1e-5)
        close(stt["var"].cpu(), var_ref.detach(), 1e-5)
        close(yd[..., :c].float().cpu(), y_ref.detach(), eps)
        # finalize + apply as ONE call (one launch when c % 8 == 0): identical statistics, identical y
        st2 = {k: torch.full((V, c), 7.0, device=DEV) for k in stt}
        yd2 = torch.zeros_like(zd)
        _lib.check(lib().gv_bn_finalize_apply_grouped_t(accum.data_ptr(), counts.data_ptr(),
                                                        gd.data_ptr() if gd is not None else None, bd.data_ptr(), 1e-3,
                                                        zd.data_ptr(), N * V, h * w, c, ld, V, 1, yd2.data_ptr(), ld,
                                                        st2["mean"].data_ptr(), st2["var"].data_ptr(),
                                                        st2["inv"].data_ptr(), st2["scale"].data_ptr(),
                                                        st2["shift"].data_ptr(), dt, st()), "finalize+apply")
        for k in stt:
            assert torch.equal(st2[k], stt[k]), k
        assert torch.equal(yd2, yd)
        assert float(yd[..., c:].float().abs().max()) == 0.0 if ld > c else True
        # backward from the ROUNDED y (its ReLU mask is what the kernel sees): take the reference mask from it too
        mask = (yd[..., :c].float().cpu() > 0).float()
        y_lin, _, _ = OB.batch_norm_train_grouped(zz, be, ga, 1e-3, groups)
        (y_lin * mask).backward(dy)
        dyd = dev(dy)
        dz = dev(q(torch.full_like(z, 0.125), tdt))     # pre-existing gradient: accumulated into
        dbeta = torch.zeros(c, device=DEV)
        dgamma = torch.zeros(c, device=DEV)
        _lib.check(lib().gv_bn_relu_bwd_sums_grouped_t(dyd.data_ptr(), ld, yd.data_ptr(), ld, zd.data_ptr(), ld,
                                                       stt["mean"].data_ptr(), stt["inv"].data_ptr(), N * V, h * w, c,
                                                       V, accum.data_ptr(), None, None, dt, st()), "bwd sums")
        _lib.check(lib().gv_bn_relu_bwd_apply_grouped_t(dyd.data_ptr(), ld, yd.data_ptr(), ld, zd.data_ptr(), ld,
                                                        stt["mean"].data_ptr(), stt["inv"].data_ptr(),
                                                        gd.data_ptr() if gd is not None else None, counts.data_ptr(),
                                                        N * V, h * w, c, V, accum.data_ptr(), dz.data_ptr(), ld,
                                                        dbeta.data_ptr(),
                                                        dgamma.data_ptr() if gd is not None else None, None, None, 1,
                                                        dt, st()),
                   "bwd apply")
        close(dz[..., :c].float().cpu() - 0.125, zz.grad, 2 * eps)
        close(dbeta.cpu(), be.grad, 1e-5)
        if gm is not None:
            close(dgamma.cpu(), ga.grad, 1e-4)
        # the engine's form: ReLU mask recomputed from z*scale + shift (y is not read), dz STORED over garbage
        dz2 = dev(q(torch.full_like(z, 77.0), tdt))
        accum2 = torch.zeros_like(accum)
        _lib.check(lib().gv_bn_relu_bwd_sums_grouped_t(dyd.data_ptr(), ld, None, 0, zd.data_ptr(), ld,
                                                       stt["mean"].data_ptr(), stt["inv"].data_ptr(), N * V, h * w, c,
                                                       V, accum2.data_ptr(), stt["scale"].data_ptr(),
                                                       stt["shift"].data_ptr(), dt, st()), "bwd sums")
        assert torch.equal(accum2, accum)
        _lib.check(lib().gv_bn_relu_bwd_apply_grouped_t(dyd.data_ptr(), ld, None, 0, zd.data_ptr(), ld,
                                                        stt["mean"].data_ptr(), stt["inv"].data_ptr(),
                                                        gd.data_ptr() if gd is not None else None, counts.data_ptr(),
                                                        N * V, h * w, c, V, accum2.data_ptr(), dz2.data_ptr(), ld, None,
                                                        None, stt["scale"].data_ptr(), stt["shift"].data_ptr(), 0, dt,
                                                        st()), "bwd apply")
        close(dz2[..., :c].float().cpu(), zz.grad, 2 * eps)


# ---- the per-view BatchNorm kernels over their launch geometries, every storage type, against fp64 (tests/bn_ref.py) ----
# name: (storage code, torch type, tolerance of y, tolerance of dz), of the tensor's scale
BN_TYPES = {"f32": (_lib.GV_F32, torch.float32, 1e-5, 1e-4), "bf16": (_lib.GV_BF16, torch.bfloat16, 2.0 ** -8, 2.0 ** -7),
            "f16": (_lib.GV_F16, torch.float16, 2.0 ** -11, 2.0 ** -10)}
# name: (N, V, h, w, c, ld).  Pixel splits (grid y) of the sums launches / of the apply launches, as the library chooses them:
BN_CASES = {
    "A": (3, 4, 7, 7, 80, 96),         # 2 / 2: 74 pixels per block, the second starts at pixel 25 of image 1; channel blocks 64 + 16
    "B": (4, 3, 10, 9, 200, 200),      # 3 / 3: 120 pixels per block; four channel blocks, the last with 8 channels
    "C": (24, 4, 1, 1, 64, 64),        # 1 / 1: hw = 1, a lane step hops 16 images on fp32 (16-bit: 24 pixels < 32 lanes, no step)
    "H": (80, 4, 1, 1, 64, 64),        # 1 / 1: hw = 1 with 80 pixels per view: several lane steps of 16 / 32 images on every type
    "D": (40, 2, 2, 2, 72, 80),        # 2 / 2: hw = 4, 80 pixels per block
    "E": (6, 5, 3, 3, 136, 136),       # 1 / 1: hw = 9, five views, ragged third channel block
    "F": (3, 4, 7, 7, 6, 7),           # 2 / 2: no 16-byte walk: the one-element walk of every type (64 channel threads x 4 pixel lanes)
    "I": (3, 4, 7, 7, 8, 9),           # 2 / 2: the channels fill a quad but the leading dimension does not: one element again
    "J": (24, 4, 1, 1, 8, 9),          # 1 / 1: hw = 1 on the one-element walk: every step of its 4 lanes hops images, 6 steps per lane
    "K": (3, 4, 7, 7, 72, 73),         # 2 / 2: two channel blocks on the one-element walk, the second with 8 channels; two pixel splits
    "G": (2, 12, 25, 32, 2048, 2048),  # 3 / 3: 534 pixels per block (ragged last), block 1 crosses into the next image at
}                                      #        pixel 800; 16-bit: 17 steps per lane = 4 unrolled trips + 1, the fold at step 12
# (case, operands start 16 bytes into their buffers, storage); G has 39 M elements: bf16 and fp32 only
BN_SWEEP = [(case, off, t) for case, off in [("A", 0), ("A", 1), ("B", 0), ("B", 1), ("C", 0), ("H", 0), ("D", 0), ("E", 0),
                                             ("F", 0), ("I", 0), ("J", 0), ("K", 0), ("G", 0)]
            for t in BN_TYPES if (case, t) != ("G", "f16")]


def _hold_totals(tag, what, acc, want0, want1):
    """The fp64 accumulator [V, c, 2] against the reference totals: 1e-6 of the largest total + 1e-9 each."""
    _hold(tag, what + "[0]", acc[..., 0], want0, 1e-6, 1e-9)
    _hold(tag, what + "[1]", acc[..., 1], want1, 1e-6, 1e-9)


def _bn_operands(case, off, tdt):
    """(z, dy) as NaN-padded slabs of values representable in the storage type, beta, gamma, counts, element offset."""
    N, V, h, w, c, ld = BN_CASES[case]
    npix = N * V * h * w
    o = off * (16 // torch.empty(0, dtype=tdt).element_size())
    g = torch.Generator(device=DEV).manual_seed(ord(case) * 2 + off)
    z = _Slab(npix, c, ld, o, tdt, NAN, (torch.randn(npix, c, generator=g, device=DEV) * 2 + 0.5).to(tdt))
    dy = _Slab(npix, c, ld, o, tdt, NAN, torch.randn(npix, c, generator=g, device=DEV).to(tdt))
    beta = torch.randn(c, generator=g, device=DEV)
    gamma = torch.rand(c, generator=g, device=DEV) + 0.5
    counts = torch.full((V,), N * h * w, dtype=torch.int32, device=DEV)
    return z, dy, beta, gamma, counts, o, g


def _bn_stats(V, c, fill=NAN):
    return {k: torch.full((V, c), fill, device=DEV) for k in ("mean", "var", "inv", "scale", "shift")}


@pytest.mark.parametrize("case,off,tname", BN_SWEEP)
def test_bn_kernels_over_their_launch_geometries_against_fp64(case, off, tname):
    """gv_bn_sums_grouped_t / gv_bn_finalize_grouped / gv_scale_shift_act_grouped_t / gv_bn_finalize_apply_grouped_t and
    gv_bn_relu_bwd_{sums,apply}_grouped_t on fp32, bf16 and fp16 storage at the geometries of BN_CASES — several pixel splits,
    blocks that start inside an image, several and ragged channel blocks, maps smaller than the pixel-lane count, the unrolled
    loop with its tail and fp32 fold, operands that are channel slices of wider buffers and start 16 bytes into them, the
    one-element walk — against the fp64 restatement of tests/bn_ref.py evaluated on the stored values, with and without gamma.
    The ReLU mask of the backward reference is taken as the kernel defines it (the stored y > 0, or float32(z*scale + shift)
    > 0 with the device's scale / shift).  Accumulators start as garbage (the sums clear them), dz / dbeta / dgamma start
    non-zero where the contract is +=, dz starts as NaN where it is stored, and nothing outside a slice may change.

    Measured worst case over all geometries (relative to the tensor's scale; bound):
                     fp32      bf16      fp16
      mean           5.1e-8    4.4e-8    4.2e-8     (1e-5)
      var            5.2e-8    7.4e-8    9.8e-8     (1e-5)
      y              1.0e-7    3.5e-3    4.2e-4     (1e-5 / 2^-8 = 3.9e-3 / 2^-11 = 4.9e-4: half an ulp at the foot of a binade)
      dz             1.4e-7    3.8e-3    4.6e-4     (1e-4 / 2^-7 = 7.8e-3 / 2^-10 = 9.8e-4)
      dz, F I J K    9.6e-8    3.8e-3    4.3e-4     (the one-element walk of the apply kernel: the same A*g + B*z + C as its quad walk)
      dbeta          8.4e-8    8.2e-8    9.1e-8     (1e-5)
      dgamma         8.3e-8    1.0e-7    9.5e-8     (1e-4)
      totals         8.1e-8    9.9e-8    1.4e-7     (1e-6; the backward ones carry the fp32 rounding of zhat)"""
    dt, tdt, tol_y, tol_dz = BN_TYPES[tname]
    N, V, h, w, c, ld = BN_CASES[case]
    nb, hw, npix = N * V, h * w, N * V * h * w
    L = lib()
    z, dy, beta, gamma, counts, o, g = _bn_operands(case, off, tdt)
    shape = (nb, hw, c)
    zs, dys = z.v.reshape(shape), dy.v.reshape(shape)            # the stored values
    pre = ((torch.rand(npix, c, generator=g, device=DEV) - 0.5) / 2).to(tdt)
    db0, dg0 = torch.randn(c, generator=g, device=DEV), torch.randn(c, generator=g, device=DEV)
    no_f32_apply = dt == _lib.GV_F32 and (c % 4 != 0 or ld % 4 != 0)   # fp32 storage has no forward apply for such a shape

    def slab(fill, values=None):
        return _Slab(npix, c, ld, o, tdt, fill, values)

    def garbage():
        return torch.full((V, c, 2), 1e30, dtype=torch.float64, device=DEV)

    for gm in (None, gamma):
        tag = "bn %s%s %s %s" % (case, "+16B" if off else "", tname, "gamma" if gm is not None else "-")
        gp = gm.data_ptr() if gm is not None else None
        # ---- forward: sums -> finalize -> apply, and the same as finalize + apply in one call
        ref = bn_ref.forward(zs, V, beta, gm, 1e-3)
        accum, stt, y = garbage(), _bn_stats(V, c), slab(SENTINEL)
        _lib.check(L.gv_bn_sums_grouped_t(z.ptr, nb, hw, c, ld, V, accum.data_ptr(), dt, st()), "sums")
        _lib.check(L.gv_bn_finalize_grouped(accum.data_ptr(), c, V, counts.data_ptr(), gp, beta.data_ptr(), 1e-3,
                                            stt["mean"].data_ptr(), stt["var"].data_ptr(), stt["inv"].data_ptr(),
                                            stt["scale"].data_ptr(), stt["shift"].data_ptr(), st()), "finalize")
        rc = L.gv_scale_shift_act_grouped_t(z.ptr, nb, hw, c, ld, stt["scale"].data_ptr(), stt["shift"].data_ptr(), V, 1,
                                            y.ptr, ld, dt, st())
        _hold_totals(tag, "sum z,z^2", accum, ref["sum_z"], ref["sum_z2"])
        _hold(tag, "mean", stt["mean"], ref["mean"], 1e-5)
        _hold(tag, "var", stt["var"], ref["var"], 1e-5)
        st2, y2 = _bn_stats(V, c, 7.0), slab(SENTINEL)
        rc2 = L.gv_bn_finalize_apply_grouped_t(accum.data_ptr(), counts.data_ptr(), gp, beta.data_ptr(), 1e-3, z.ptr, nb, hw,
                                               c, ld, V, 1, y2.ptr, ld, st2["mean"].data_ptr(), st2["var"].data_ptr(),
                                               st2["inv"].data_ptr(), st2["scale"].data_ptr(), st2["shift"].data_ptr(), dt,
                                               st())
        for k in stt:
            assert torch.equal(st2[k], stt[k]), k
        if no_f32_apply:
            assert rc == _lib.GV_E_ALIGN and rc2 == _lib.GV_E_ALIGN
            assert bool((y.buf == SENTINEL).all()) and bool((y2.buf == SENTINEL).all())
            # the activation such a layer would keep: one rounding of z*scale + shift with the device's scale / shift
            lin = zs.double().reshape(N, V, hw, c) * stt["scale"].double()[None, :, None, :] + \
                stt["shift"].double()[None, :, None, :]
            y.v.copy_(lin.float().clamp_min(0.0).reshape(npix, c))
        else:
            _lib.check(rc, "apply")
            _lib.check(rc2, "finalize + apply")
            _hold(tag, "y", y.v, ref["y"].reshape(npix, c), tol_y)
            assert torch.equal(y2.buf, y.buf) and y.outside_intact()
        # ---- backward from the kept activation: its mask is the stored y > 0; dz, dbeta, dgamma are accumulated into
        ys = y.v.reshape(shape)
        rb = bn_ref.backward(zs, dys, ys > 0, V, gm, 1e-3)
        acc_y, dz = garbage(), slab(SENTINEL, pre)
        dbeta, dgamma = db0.clone(), dg0.clone()
        _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy.ptr, ld, y.ptr, ld, z.ptr, ld, stt["mean"].data_ptr(),
                                                   stt["inv"].data_ptr(), nb, hw, c, V, acc_y.data_ptr(), None, None, dt,
                                                   st()), "bwd sums (kept y)")
        _lib.check(L.gv_bn_relu_bwd_apply_grouped_t(dy.ptr, ld, y.ptr, ld, z.ptr, ld, stt["mean"].data_ptr(),
                                                    stt["inv"].data_ptr(), gp, counts.data_ptr(), nb, hw, c, V,
                                                    acc_y.data_ptr(), dz.ptr, ld, dbeta.data_ptr(),
                                                    dgamma.data_ptr() if gm is not None else None, None, None, 1, dt, st()),
                   "bwd apply (kept y)")
        _hold_totals(tag, "sum g,gzh", acc_y, rb["sum_g"], rb["sum_gzh"])
        _hold(tag, "dz", dz.v.double() - pre.double(), rb["dz"].reshape(npix, c), tol_dz)
        _hold(tag, "dbeta", dbeta.double() - db0.double(), rb["dbeta"], 1e-5)
        if gm is not None:
            _hold(tag, "dgamma", dgamma.double() - dg0.double(), rb["dgamma"], 1e-4)
        else:
            assert torch.equal(dgamma, dg0)
        assert dz.outside_intact()
        # ---- the engine's form: mask recomputed from z (y is not read), dz STORED over NaN
        rz = bn_ref.backward(zs, dys, bn_ref.mask_from_z(zs, V, stt["scale"], stt["shift"]), V, gm, 1e-3)
        acc_z, dz2, dz3 = garbage(), slab(SENTINEL), slab(SENTINEL)
        dz2.v.fill_(NAN)
        dz3.v.zero_()
        _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy.ptr, ld, None, 0, z.ptr, ld, stt["mean"].data_ptr(),
                                                   stt["inv"].data_ptr(), nb, hw, c, V, acc_z.data_ptr(),
                                                   stt["scale"].data_ptr(), stt["shift"].data_ptr(), dt, st()),
                   "bwd sums (mask from z)")
        _hold_totals(tag, "sum g,gzh", acc_z, rz["sum_g"], rz["sum_gzh"])
        # Both masks select the same elements (an fp16 y may underflow to 0 where z*scale + shift > 0: fp16 has the two
        # comparisons with the reference above instead), so the two sums are the same bits — where the sums are order-
        # independent at all, i.e. inside the exactness range of their fixed grid: 2^13 on 16-bit storage, 2 on fp32.  fp32
        # sums of three splits beyond it differ by the rounding of three fp64 additions (<= 2^-50 of sum |g|, asserted;
        # measured 1.2e-16 on cases B and G, 0 elsewhere), so fp32 repeats the two launches with dy * 2^-10.
        bound = torch.stack([rb["sum_abs_g"], rb["sum_abs_gzh"]], dim=-1)
        print("%s kept-y vs recomputed sums: max |diff| / sum|g| %.3e" % (tag, float(((acc_z - acc_y).abs() / bound.clamp_min(1e-300)).max())))
        if tname == "bf16":
            assert float(bound.max()) < 2.0 ** 13 and torch.equal(acc_z, acc_y)
        elif tname == "f32":
            assert bool(((acc_z - acc_y).abs() <= 2.0 ** -50 * bound).all())
            assert float(bound.max()) * 2.0 ** -10 < 2.0
            dy_s, acc_ys, acc_zs = slab(NAN, dy.v * 2.0 ** -10), garbage(), garbage()
            for a, yp, sp, hp in ((acc_ys, y.ptr, None, None), (acc_zs, None, stt["scale"].data_ptr(), stt["shift"].data_ptr())):
                _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy_s.ptr, ld, yp, ld if yp else 0, z.ptr, ld,
                                                           stt["mean"].data_ptr(), stt["inv"].data_ptr(), nb, hw, c, V,
                                                           a.data_ptr(), sp, hp, dt, st()), "bwd sums (dy * 2^-10)")
            assert torch.equal(acc_zs, acc_ys)
            _hold_totals(tag, "sum g,gzh", acc_zs, rz["sum_g"] * 2.0 ** -10, rz["sum_gzh"] * 2.0 ** -10)
        for out, accumulate in ((dz2, 0), (dz3, 1)):
            _lib.check(L.gv_bn_relu_bwd_apply_grouped_t(dy.ptr, ld, None, 0, z.ptr, ld, stt["mean"].data_ptr(),
                                                        stt["inv"].data_ptr(), gp, counts.data_ptr(), nb, hw, c, V,
                                                        acc_z.data_ptr(), out.ptr, ld, None, None, stt["scale"].data_ptr(),
                                                        stt["shift"].data_ptr(), accumulate, dt, st()),
                       "bwd apply (mask from z)")
        _hold(tag, "dz", dz2.v, rz["dz"].reshape(npix, c), tol_dz)
        assert torch.equal(dz2.v, dz3.v)                         # a store is an accumulation into zeros
        assert dz2.outside_intact() and dz3.outside_intact()
    assert z.outside_intact() and dy.outside_intact()


@pytest.mark.parametrize("case,tname", [(case, t) for case in "ABG" for t in BN_TYPES if (case, t) != ("G", "f16")])
def test_bn_split_sums_do_not_depend_on_the_order_of_their_blocks(case, tname):
    """The blocks of a sums launch round their partials to a fixed grid before the fp64 atomics, so inside the documented
    ranges (fp32 storage: sum z < 2^13, sum z^2 < 2^17, backward < 2; 16-bit: 2^23 / 2^29 / 2^13) every addition is exact and
    two runs give the same bits whatever order the 2 or 3 pixel splits arrive in.  That the inputs ARE inside the ranges is
    asserted from the reference's totals of absolute values, which bound every partial sum."""
    dt, tdt, _, _ = BN_TYPES[tname]
    N, V, h, w, c, ld = BN_CASES[case]
    nb, hw = N * V, h * w
    L = lib()
    z, dy, beta, _, counts, _, _ = _bn_operands(case, 0, tdt)
    if dt == _lib.GV_F32:
        dy.v.mul_(2.0 ** -10)                                    # (a power of two: still exact values)
    zs, dys = z.v.reshape(nb, hw, c), dy.v.reshape(nb, hw, c)
    lim_z, lim_z2, lim_b = (2.0 ** 13, 2.0 ** 17, 2.0) if dt == _lib.GV_F32 else (2.0 ** 23, 2.0 ** 29, 2.0 ** 13)
    ref = bn_ref.forward(zs, V, beta, None, 1e-3)
    assert float(ref["sum_abs_z"].max()) < lim_z and float(ref["sum_z2"].max()) < lim_z2
    acc = [torch.full((V, c, 2), 1e30, dtype=torch.float64, device=DEV) for _ in range(2)]
    for a in acc:
        _lib.check(L.gv_bn_sums_grouped_t(z.ptr, nb, hw, c, ld, V, a.data_ptr(), dt, st()), "sums")
    assert torch.equal(acc[0], acc[1])
    stt = _bn_stats(V, c)
    _lib.check(L.gv_bn_finalize_grouped(acc[0].data_ptr(), c, V, counts.data_ptr(), None, beta.data_ptr(), 1e-3,
                                        stt["mean"].data_ptr(), stt["var"].data_ptr(), stt["inv"].data_ptr(),
                                        stt["scale"].data_ptr(), stt["shift"].data_ptr(), st()), "finalize")
    rz = bn_ref.backward(zs, dys, bn_ref.mask_from_z(zs, V, stt["scale"], stt["shift"]), V, None, 1e-3)
    assert float(rz["sum_abs_g"].max()) < lim_b and float(rz["sum_abs_gzh"].max()) < lim_b
    accb = [torch.full((V, c, 2), 1e30, dtype=torch.float64, device=DEV) for _ in range(2)]
    for a in accb:
        _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy.ptr, ld, None, 0, z.ptr, ld, stt["mean"].data_ptr(),
                                                   stt["inv"].data_ptr(), nb, hw, c, V, a.data_ptr(), stt["scale"].data_ptr(),
                                                   stt["shift"].data_ptr(), dt, st()), "bwd sums")
    assert torch.equal(accb[0], accb[1])
    _hold_totals("order %s %s" % (case, tname), "sum g,gzh", accb[0], rz["sum_g"], rz["sum_gzh"])


@pytest.mark.parametrize("layout", ["ld9", "off1"])
@pytest.mark.parametrize("tname", list(BN_TYPES))
def test_bn_apply_does_not_depend_on_the_width_it_is_walked_at(tname, layout):
    """The apply does not depend on the width it is walked at: the same stored z and dy, the same accumulators and the same
    statistics, once in a layout the quad walk takes (c = 8, ld = 8, 16-byte aligned) and once in one it declines (ld = 9, or
    the base one element off), give the same bits — y of gv_scale_shift_act_grouped_t, y and the five statistics of
    gv_bn_finalize_apply_grouped_t, and dz (stored and accumulated), dbeta and dgamma of gv_bn_relu_bwd_apply_grouped_t with
    the kept y, with the recomputed mask and, on 16-bit storage, with GV_ACCUM_RAW_Z accumulators.  Both layouts are fed from
    ONE sums launch (the sums themselves depend on the thread layout, legitimately).  fp32 storage has no forward apply for
    the second layout (GV_E_ALIGN), so it covers the backward, with the y of the first."""
    dt, tdt, _, _ = BN_TYPES[tname]
    N, V, h, w, c = 3, 4, 7, 7, 8
    nb, hw, npix = N * V, h * w, N * V * h * w
    L = lib()
    g = torch.Generator(device=DEV).manual_seed(11)
    zv = (torch.randn(npix, c, generator=g, device=DEV) * 2 + 0.5).to(tdt)
    dyv = torch.randn(npix, c, generator=g, device=DEV).to(tdt)
    pre = ((torch.rand(npix, c, generator=g, device=DEV) - 0.5) / 2).to(tdt)
    beta, gamma = torch.randn(c, generator=g, device=DEV), torch.rand(c, generator=g, device=DEV) + 0.5
    db0, dg0 = torch.randn(c, generator=g, device=DEV), torch.randn(c, generator=g, device=DEV)
    counts = torch.full((V,), N * hw, dtype=torch.int32, device=DEV)
    lays = [(8, 0), (9, 0) if layout == "ld9" else (8, 1)]          # (ld, element offset of the base)

    def slab(lay, fill, values=None):
        return _Slab(npix, c, lay[0], lay[1], tdt, fill, values)

    def garbage():
        return torch.full((V, c, 2), 1e30, dtype=torch.float64, device=DEV)

    z, dy = [slab(lay, NAN, zv) for lay in lays], [slab(lay, NAN, dyv) for lay in lays]
    assert z[0].ptr % 16 == 0 and dy[0].ptr % 16 == 0 and (z[1].ptr % 16 != 0 or layout == "ld9")
    accum, stt = garbage(), _bn_stats(V, c)
    _lib.check(L.gv_bn_sums_grouped_t(z[0].ptr, nb, hw, c, 8, V, accum.data_ptr(), dt, st()), "sums")
    _lib.check(L.gv_bn_finalize_grouped(accum.data_ptr(), c, V, counts.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-3,
                                        stt["mean"].data_ptr(), stt["var"].data_ptr(), stt["inv"].data_ptr(),
                                        stt["scale"].data_ptr(), stt["shift"].data_ptr(), st()), "finalize")
    mean, inv, scale, shift = (stt[k].data_ptr() for k in ("mean", "inv", "scale", "shift"))
    # ---- forward
    ys, fused = [], []
    for zz, (ld, _) in zip(z, lays):
        y, y2, st2 = slab((ld, _), SENTINEL), slab((ld, _), SENTINEL), _bn_stats(V, c, 7.0)
        rc = L.gv_scale_shift_act_grouped_t(zz.ptr, nb, hw, c, ld, scale, shift, V, 1, y.ptr, ld, dt, st())
        rc2 = L.gv_bn_finalize_apply_grouped_t(accum.data_ptr(), counts.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-3,
                                               zz.ptr, nb, hw, c, ld, V, 1, y2.ptr, ld, st2["mean"].data_ptr(),
                                               st2["var"].data_ptr(), st2["inv"].data_ptr(), st2["scale"].data_ptr(),
                                               st2["shift"].data_ptr(), dt, st())
        if dt == _lib.GV_F32 and zz is z[1]:
            assert rc == _lib.GV_E_ALIGN and rc2 == _lib.GV_E_ALIGN
            y.v.copy_(ys[0].v)                                   # (the kept activation of the backward below)
        else:
            _lib.check(rc, "apply")
            _lib.check(rc2, "finalize + apply")
            assert torch.equal(y2.buf, y.buf) and y.outside_intact()
        for k in stt:
            assert torch.equal(st2[k], stt[k]), k
        ys.append(y)
        fused.append(y2)
    assert torch.equal(ys[1].v, ys[0].v)
    if dt != _lib.GV_F32:
        assert torch.equal(fused[1].v, fused[0].v)
    # ---- backward: the sums once, from the first layout
    acc_y, acc_z = garbage(), garbage()
    _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy[0].ptr, 8, ys[0].ptr, 8, z[0].ptr, 8, mean, inv, nb, hw, c, V,
                                               acc_y.data_ptr(), None, None, dt, st()), "bwd sums (kept y)")
    _lib.check(L.gv_bn_relu_bwd_sums_grouped_t(dy[0].ptr, 8, None, 0, z[0].ptr, 8, mean, inv, nb, hw, c, V,
                                               acc_z.data_ptr(), scale, shift, dt, st()), "bwd sums (mask from z)")
    forms = [("kept y", acc_y, True, 0), ("mask from z", acc_z, False, 0)]
    if dt != _lib.GV_F32:
        # the raw accumulator a fused data gradient would have produced: sum g, sum g*z (test_gpu_bn_fusion.py)
        zf, dyf = zv.double().reshape(nb, hw, c), dyv.double().reshape(nb, hw, c)
        grp = torch.arange(nb, device=DEV) % V
        gg = dyf * (zf * stt["scale"][grp][:, None, :].double() + stt["shift"][grp][:, None, :].double() > 0).double()
        raw = torch.zeros(V, c, 2, dtype=torch.float64, device=DEV)
        for v in range(V):
            raw[v, :, 0] = gg[grp == v].reshape(-1, c).sum(0)
            raw[v, :, 1] = (gg * zf)[grp == v].reshape(-1, c).sum(0)
        forms.append(("raw z", raw, False, _lib.GV_ACCUM_RAW_Z))
    for name, acc, kept, flag in forms:
        for accumulate in (0, 1):
            outs = []
            for i, (ld, _) in enumerate(lays):
                dz = slab(lays[i], SENTINEL, pre)
                if not accumulate:
                    dz.v.fill_(NAN)
                dbeta, dgamma = db0.clone(), dg0.clone()
                _lib.check(L.gv_bn_relu_bwd_apply_grouped_t(
                    dy[i].ptr, ld, ys[i].ptr if kept else None, ld if kept else 0, z[i].ptr, ld, mean, inv, gamma.data_ptr(),
                    counts.data_ptr(), nb, hw, c, V, acc.data_ptr(), dz.ptr, ld, dbeta.data_ptr(), dgamma.data_ptr(),
                    None if kept else scale, None if kept else shift, accumulate, dt | flag, st()), "bwd apply (%s)" % name)
                assert dz.outside_intact()
                outs.append((dz.v.clone(), dbeta, dgamma))
            what = "%s %s %s %s" % (tname, layout, name, "accumulated" if accumulate else "stored")
            assert torch.equal(outs[1][0], outs[0][0]), "dz " + what          # (equal also says: no NaN left)
            assert torch.equal(outs[1][1], outs[0][1]) and not torch.equal(outs[0][1], db0), "dbeta " + what
            assert torch.equal(outs[1][2], outs[0][2]) and not torch.equal(outs[0][2], dg0), "dgamma " + what


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("k,stride,padding,mode", [(3, 2, "VALID", "max"), (3, 2, "SAME", "max"),
                                                    (3, 1, "SAME", "avg"), (1, 2, "VALID", "max"),
                                                    (3, 1, "SAME", "max")])
@pytest.mark.parametrize("c", [16, 12])
def test_pool_backward_typed(dt, tdt, eps, k, stride, padding, mode, c):
    g = torch.Generator().manual_seed(1)
    x = q(torch.randn(2, 9, 8, c, generator=g), tdt)
    x[0, 2:5, 2:5, :] = 0.5                              # ties: the first maximum in scan order takes the gradient
    x = x.requires_grad_(True)
    y = OB.max_pool2d(x, k, stride, padding) if mode == "max" else OB.avg_pool2d_same3(x)
    dy = q(torch.randn(*y.shape, generator=g), tdt)
    y.backward(dy)
    pt = OB.same_pads(9, k, stride)[0] if padding == "SAME" else 0
    pl = OB.same_pads(8, k, stride)[0] if padding == "SAME" else 0
    d = _lib.PoolDesc(2, 9, 8, c, c, k, k, stride, pt, pl, y.shape[1], y.shape[2], c,
                      _lib.GV_POOL_MAX if mode == "max" else _lib.GV_POOL_AVG, dt)
    xd, dyd = x.detach().to(tdt).to(DEV), dy.to(tdt).to(DEV)
    dx = torch.full_like(xd, 0.25)
    _lib.check(lib().gv_pool2d_bwd(C.byref(d), xd.data_ptr(), dyd.data_ptr(), c, dx.data_ptr(), c, st()), "pool_bwd")
    # the fp32 kernel on the same inputs picks the same winners (ties included)
    d32 = _lib.PoolDesc(2, 9, 8, c, c, k, k, stride, pt, pl, y.shape[1], y.shape[2], c,
                        _lib.GV_POOL_MAX if mode == "max" else _lib.GV_POOL_AVG, _lib.GV_F32)
    x32, dy32 = x.detach().to(DEV), dy.to(DEV)
    dx32 = torch.zeros_like(x32)
    _lib.check(lib().gv_pool2d_bwd(C.byref(d32), x32.data_ptr(), dy32.data_ptr(), c, dx32.data_ptr(), c, st()), "pool_bwd")
    close(dx.float().cpu() - 0.25, dx32.cpu(), 2 * eps)
    # store form (the first contribution to a gradient): dx = ..., whatever dx held
    d.mode |= _lib.GV_POOL_BWD_STORE
    dxs = torch.full_like(xd, float("nan"))
    _lib.check(lib().gv_pool2d_bwd(C.byref(d), xd.data_ptr(), dyd.data_ptr(), c, dxs.data_ptr(), c, st()), "pool_bwd")
    close(dxs.float().cpu(), dx32.cpu(), eps)
    if mode == "avg" or (k, stride) != (3, 1):
        close(dx32.cpu(), x.grad, 1e-5)                  # (torch splits differently only where windows tie)


@pytest.mark.parametrize("dt,tdt", [(_lib.GV_BF16, torch.bfloat16), (_lib.GV_F16, torch.float16), (_lib.GV_F32, torch.float32)])
@pytest.mark.parametrize("k,stride,padding", [(3, 2, "VALID"), (3, 2, "SAME"), (3, 1, "SAME"), (1, 2, "VALID"), (2, 2, "VALID")])
@pytest.mark.parametrize("c,ld", [(16, 16), (24, 40), (5, 7)])
@pytest.mark.parametrize("hw", [(11, 9), (12, 10)])      # (an even map: TF's SAME 3x3 / 2 pads (0, 1) there — ResNet-v2's pool1)
def test_max_pool_with_recorded_argmax(dt, tdt, k, stride, padding, c, ld, hw):
    """gv_pool2d_fwd_argmax / gv_pool2d_bwd_argmax (the training step's max pools): the forward output is that of
    gv_pool2d_fwd bit for bit, the recorded byte is the row-major tap of the FIRST maximum of the window (ties planted),
    and the backward, which never sees x, reproduces gv_pool2d_bwd (tf MaxPoolGrad) bit for bit in both its accumulate and
    its store form."""
    g = torch.Generator().manual_seed(k * 10 + stride + c)
    nb, (ih, iw) = 2, hw
    x = q(torch.randn(nb, ih, iw, c, generator=g), tdt)
    x[0, 2:6, 2:6, :] = 0.5                              # ties
    x[1, :, :, 0] = -3.0
    pt = OB.same_pads(ih, k, stride)[0] if padding == "SAME" else 0
    pl = OB.same_pads(iw, k, stride)[0] if padding == "SAME" else 0
    yref = OB.max_pool2d(x, k, stride, padding)
    oh, ow = yref.shape[1], yref.shape[2]
    xd = torch.zeros(nb, ih, iw, ld, dtype=tdt, device=DEV)
    xd[..., :c] = x.to(tdt).to(DEV)
    d = _lib.PoolDesc(nb, ih, iw, c, ld, k, k, stride, pt, pl, oh, ow, ld, _lib.GV_POOL_MAX, dt)
    y0 = torch.zeros(nb, oh, ow, ld, dtype=tdt, device=DEV)
    y1 = torch.zeros_like(y0)
    arg = torch.full((nb, oh, ow, c), 255, dtype=torch.uint8, device=DEV)
    _lib.check(lib().gv_pool2d_fwd(C.byref(d), xd.data_ptr(), y0.data_ptr(), st()), "pool")
    _lib.check(lib().gv_pool2d_fwd_argmax(C.byref(d), xd.data_ptr(), y1.data_ptr(), arg.data_ptr(), st()), "pool+argmax")
    assert torch.equal(y0, y1) and torch.equal(y1[..., :c].float().cpu(), yref)
    # the first maximum in scan order, by hand
    xp = torch.full((nb, ih + 2 * k, iw + 2 * k, c), float("-inf"))
    xp[:, pt:pt + ih, pl:pl + iw] = x
    want = torch.zeros(nb, oh, ow, c, dtype=torch.uint8)
    for oy in range(oh):
        for ox in range(ow):
            win = xp[:, oy * stride:oy * stride + k, ox * stride:ox * stride + k].reshape(nb, k * k, c)
            want[:, oy, ox] = (win == win.max(dim=1, keepdim=True).values).to(torch.uint8).argmax(dim=1).to(torch.uint8)
    assert torch.equal(arg.cpu(), want)
    dy = torch.zeros(nb, oh, ow, ld, dtype=tdt, device=DEV)
    dy[..., :c] = q(torch.randn(nb, oh, ow, c, generator=g), tdt).to(tdt).to(DEV)
    for store in (0, _lib.GV_POOL_BWD_STORE):            # (both entry points have the store form for every storage type)
        d.mode = _lib.GV_POOL_MAX | store
        dx0 = torch.full((nb, ih, iw, ld), 0.25, dtype=tdt, device=DEV)
        dx1 = dx0.clone()
        _lib.check(lib().gv_pool2d_bwd(C.byref(d), xd.data_ptr(), dy.data_ptr(), ld, dx0.data_ptr(), ld, st()), "pool_bwd")
        _lib.check(lib().gv_pool2d_bwd_argmax(C.byref(d), arg.data_ptr(), dy.data_ptr(), ld, dx1.data_ptr(), ld, st()),
                   "pool_bwd (argmax)")
        assert torch.equal(dx0[..., :c], dx1[..., :c])
        assert (dx1[..., c:] == 0.25).all()


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
def test_accumulate_and_bias_grad_typed(dt, tdt, eps):
    g = torch.Generator().manual_seed(5)
    for c, ld in ((64, 64), (24, 40), (5, 7)):
        src = q(torch.randn(37, c, generator=g), tdt)
        dst = q(torch.randn(37, c, generator=g), tdt)
        sd = torch.zeros(37, ld, dtype=tdt, device=DEV)
        dd = torch.zeros(37, ld, dtype=tdt, device=DEV)
        sd[:, :c], dd[:, :c] = src.to(tdt).to(DEV), dst.to(tdt).to(DEV)
        _lib.check(lib().gv_accumulate_t(sd.data_ptr(), ld, dd.data_ptr(), ld, 37, c, dt, st()), "acc")
        close(dd[:, :c].float().cpu(), src + dst, eps)
        accum = torch.zeros(2 * c, dtype=torch.float64, device=DEV)
        db = torch.full((c,), 0.5, device=DEV)
        _lib.check(lib().gv_bias_grad_t(sd.data_ptr(), ld, 37, c, accum.data_ptr(), db.data_ptr(), dt, st()), "bias")
        close(db.cpu() - 0.5, src.sum(0), 1e-5)


@pytest.mark.parametrize("tname", list(BN_TYPES))
@pytest.mark.parametrize("c,ld", [(72, 80), (5, 7), (8, 9)])
def test_bias_grad_over_several_pixel_splits(tname, c, ld):
    """gv_bias_grad_t with more than one pixel split (fp32: 2100 pixels = 2 workgroups of 2048; 16-bit: 300 pixels = 3 of
    128), on the streaming and on the scalar kernel, a slice of a wider buffer whose other channels hold NaN: dbias, which
    starts non-zero, grows by the fp64 column sums (bound 1e-5 of their scale; measured 3.4e-8 / 4.0e-8 / 4.2e-8 on fp32 /
    bf16 / fp16)."""
    dt, tdt, _, _ = BN_TYPES[tname]
    npix = 2100 if dt == _lib.GV_F32 else 300
    g = torch.Generator(device=DEV).manual_seed(c)
    dz = _Slab(npix, c, ld, 0, tdt, NAN, torch.randn(npix, c, generator=g, device=DEV).to(tdt))
    db0 = torch.randn(c, generator=g, device=DEV)
    db = db0.clone()
    accum = torch.full((2 * c,), 1e30, dtype=torch.float64, device=DEV)
    _lib.check(lib().gv_bias_grad_t(dz.ptr, ld, npix, c, accum.data_ptr(), db.data_ptr(), dt, st()), "bias")
    _hold("bias %s c=%d" % (tname, c), "dbias", db.double() - db0.double(), dz.v.double().sum(0), 1e-5)
    assert dz.outside_intact()


@pytest.mark.parametrize("tname", list(BN_TYPES))
@pytest.mark.parametrize("c,ld", [(72, 80), (5, 7), (8, 9)])
def test_accumulate_is_the_exact_sum_rounded_once(tname, c, ld):
    """gv_accumulate_t at 300 pixels (more than one workgroup), vector and scalar kernel, slices of wider buffers: dst is the
    sum formed in fp64 and rounded once to the storage type, bit for bit; the other channels of dst keep their sentinel."""
    dt, tdt, _, _ = BN_TYPES[tname]
    npix = 300
    g = torch.Generator(device=DEV).manual_seed(c + 1)
    src = _Slab(npix, c, ld, 0, tdt, NAN, torch.randn(npix, c, generator=g, device=DEV).to(tdt))
    dst = _Slab(npix, c, ld, 0, tdt, SENTINEL, torch.randn(npix, c, generator=g, device=DEV).to(tdt))
    want = (src.v.double() + dst.v.double()).to(tdt)
    _lib.check(lib().gv_accumulate_t(src.ptr, ld, dst.ptr, ld, npix, c, dt, st()), "acc")
    assert torch.equal(dst.v, want)
    assert dst.outside_intact() and src.outside_intact()


CONVS =[((3, 3), 1, "SAME", 32, 48, 3, 12, 11), ((3, 3), 2, "VALID", 32, 64, 3, 12, 11),
         ((1, 7), 1, "SAME", 48, 32, 3, 12, 11), ((5, 5), 1, "SAME", 48, 64, 3, 12, 11),
         ((3, 3), 1, "VALID", 80, 96, 3, 12, 11), ((1, 1), 1, "SAME", 96, 32, 3, 12, 11),
         ((3, 3), 2, (1, 1, 1, 1), 64, 64, 3, 12, 11), ((1, 1), 2, "VALID", 64, 128, 3, 12, 11),
         ((3, 3), 2, "VALID", 3, 32, 3, 12, 11),                 # stem: fp32-MFMA kernel with typed loads
         ((3, 3), 1, "SAME", 288, 384, 2, 9, 9), ((1, 1), 1, "SAME", 768, 192, 4, 12, 12),
         ((7, 1), 1, "SAME", 128, 192, 5, 12, 12), ((3, 3), 1, "SAME", 200, 136, 2, 7, 7),
         ((3, 3), 1, "VALID", 32, 64, 18, 111, 111),             # few-channel stem layers at full width (strips of 28)
         ((3, 3), 1, "VALID", 32, 32, 3, 40, 37), ((1, 3), 1, "SAME", 384, 384, 7, 5, 5),
         ((3, 1), 1, "SAME", 96, 32, 4, 17, 17), ((3, 3), 1, "SAME", 64, 96, 3, 35, 35)]


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("k,stride,padding,cin,cout,nb,ih,iw", CONVS)
def test_conv_wgrad_and_dgrad_typed(dt, tdt, eps, k, stride, padding, cin, cout, nb, ih, iw):
    g = torch.Generator().manual_seed(hash((k, stride, cin)) % 997)
    x = q(torch.randn(nb, ih, iw, cin, generator=g), tdt).requires_grad_(True)
    w = q(torch.randn(k[0], k[1], cin, cout, generator=g) * 0.1, tdt).requires_grad_(True)
    big = nb * ih * iw > 100000
    dev = DEV if big else "cpu"
    z = OB.conv2d(x.to(dev), w.to(dev), stride, padding) if big else OB.conv2d(x, w, stride, padding)
    dz = q(torch.randn(*z.shape, generator=g), tdt)
    z.backward(dz.to(z.device))
    oh, ow = z.shape[1:3]
    if isinstance(padding, str):
        pt = OB.same_pads(ih, k[0], stride)[0] if padding == "SAME" else 0
        pl = OB.same_pads(iw, k[1], stride)[0] if padding == "SAME" else 0
    else:
        pt, pl = padding[0], padding[2]
    # operands inside wider buffers (a concat slice): pixel strides larger than the channel counts
    xld, zld = (cin + 8 if cin % 8 == 0 else cin), cout + 16
    xd = torch.zeros(nb, ih, iw, xld, dtype=tdt, device=DEV)
    xd[..., :cin] = x.detach().to(tdt).to(DEV)
    dzd = torch.zeros(nb, oh, ow, zld, dtype=tdt, device=DEV)
    dzd[..., :cout] = dz.to(tdt).to(DEV)
    dw = torch.full((k[0], k[1], cin, cout), 0.5, device=DEV)
    d = _lib.ConvDesc(nb, ih, iw, cin, xld, k[0], k[1], stride, pt, pl, oh, ow, cout, cout, 0, 0, 0, dt, 0, 0, 0, 0)
    _lib.check(lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), zld, dw.data_ptr(), st()), "wgrad")
    # products of 16-bit values are exact in fp32: only the summation order differs from autograd
    close(dw.cpu() - 0.5, w.grad, 3e-5 if not big else 2e-4)
    if cin % 16 or big:
        return
    wt = torch.flip(w.detach(), (0, 1)).permute(0, 1, 3, 2).contiguous().to(DEV)
    n = lib().gv_packed_filter_bytes(k[0], k[1], cout, cin, dt, 0)
    wp = torch.empty(n, dtype=torch.uint8, device=DEV)
    _lib.check(lib().gv_pack_filter_hwio(wt.data_ptr(), k[0], k[1], cout, cin, wp.data_ptr(), dt, 0, st()), "pack")
    dx = torch.full((nb, ih, iw, xld), 0.25, dtype=tdt, device=DEV)
    ones, zeros = torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV)
    dd = _lib.ConvDesc(nb, oh, ow, cout, zld, k[0], k[1], 1, k[0] - 1 - pt, k[1] - 1 - pl, ih, iw, cin, xld, xld, 0,
                       0, dt, 0, 0, 0, stride if stride > 1 else 0)
    _lib.check(lib().gv_conv2d_fwd(C.byref(dd), dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(),
                                   dx.data_ptr(), dx.data_ptr(), None, None, None, st()), "dgrad")
    close(dx[..., :cin].float().cpu() - 0.25, x.grad, 2 * eps)
    assert float((dx[..., cin:].float() - 0.25).abs().max()) == 0.0     # neighbours in the wider buffer untouched


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
def test_wgrad_mfma_kernel_equals_the_fp32_mfma_kernel_on_typed_loads(dt, tdt, eps):
    """Two independent implementations of the 16-bit filter gradient (transposed-LDS-read 16-bit MFMA vs fp32 MFMA
    with typed loads) agree to summation order."""
    g = torch.Generator().manual_seed(11)
    nb, ih, iw, cin, cout = 6, 17, 17, 160, 192
    x = torch.randn(nb, ih, iw, cin, generator=g).to(tdt).to(DEV)
    dz = torch.randn(nb, ih, iw, cout, generator=g).to(tdt).to(DEV)
    outs = []
    for f32 in (0, 1):
        lib().gv_conv2d_wgrad_set_lp_f32(f32)
        dw = torch.zeros(1, 7, cin, cout, device=DEV)
        d = _lib.ConvDesc(nb, ih, iw, cin, cin, 1, 7, 1, 0, 3, ih, iw, cout, cout, 0, 0, 0, dt, 0, 0, 0, 0)
        _lib.check(lib().gv_conv2d_wgrad(C.byref(d), x.data_ptr(), dz.data_ptr(), cout, dw.data_ptr(), st()), "wgrad")
        outs.append(dw.cpu())
    lib().gv_conv2d_wgrad_set_lp_f32(0)
    close(outs[0], outs[1], 2e-5)


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
def test_wgrad_every_launch_configuration(dt, tdt, eps):
    """gv_conv_desc.tile_cfg of the 16-bit filter gradient (tap-per-workgroup tiles x pixel split, strip form x
    workgroup count; a speed choice): same result."""
    g = torch.Generator().manual_seed(12)
    nb, ih, iw, cin, cout = 5, 13, 12, 96, 160
    x = torch.randn(nb, ih, iw, cin, generator=g).to(tdt).to(DEV)
    dz = torch.randn(nb, ih, iw, cout, generator=g).to(tdt).to(DEV)
    n = lib().gv_conv2d_wgrad_num_cfgs(dt)
    assert n == 96 and lib().gv_conv2d_wgrad_num_cfgs(_lib.GV_F32) == 0       # 27 tiles + 3 strip + 61 LDS-DMA + 5 deep strip
    outs = []
    for cfg in range(n + 1):
        dw = torch.zeros(3, 3, cin, cout, device=DEV)
        d = _lib.ConvDesc(nb, ih, iw, cin, cin, 3, 3, 1, 1, 1, ih, iw, cout, cout, 0, 0, 0, dt, 0, cfg, 0, 0)
        _lib.check(lib().gv_conv2d_wgrad(C.byref(d), x.data_ptr(), dz.data_ptr(), cout, dw.data_ptr(), st()), "wgrad")
        outs.append(dw.cpu())
    for o in outs[1:]:
        close(o, outs[0], 2e-5)
    d = _lib.ConvDesc(nb, ih, iw, cin, cin, 3, 3, 1, 1, 1, ih, iw, cout, cout, 0, 0, 0, dt, 0, n + 1, 0, 0)
    assert lib().gv_conv2d_wgrad(C.byref(d), x.data_ptr(), dz.data_ptr(), cout, outs[0].to(DEV).data_ptr(), st()) != 0


WGRAD_DMA_CFGS = [31, 32, 33, 34, 38, 42, 55, 56, 57, 58, 59, 64, 65, 68, 69, 73, 74, 77, 78, 82, 86, 91]


@pytest.mark.parametrize("k,stride,padding,cin,cout,nb,ih,iw", [c for c in CONVS if c[5] * c[6] * c[7] < 100000])
def test_wgrad_lds_dma_form_on_every_layer_class(k, stride, padding, cin, cout, nb, ih, iw):
    """The LDS-DMA staged filter gradient (csrc/wgrad_dma.hip; tile_cfg 31..64: 64- / 128- / 192-channel tile sides): strided and padded layers, channel
    counts that do not fill a tile, ragged pixel slices, operands that are channel slices of wider buffers — against
    autograd on the same 16-bit values (exact products: only the summation order differs)."""
    dt, tdt, eps = TYPES[0]
    if cin % 8 or cout % 8:
        pytest.skip("the 16-bit MFMA filter gradient needs whole 8-channel chunks")
    # (every tile configuration on ONE set of operands: allocation and the oracle's convolution dominate a case, not the launch)
    g = torch.Generator().manual_seed(hash((k, stride, cin)) % 997)
    x = q(torch.randn(nb, ih, iw, cin, generator=g), tdt).requires_grad_(True)
    w = q(torch.randn(k[0], k[1], cin, cout, generator=g) * 0.1, tdt).requires_grad_(True)
    z = OB.conv2d(x, w, stride, padding)
    dz = q(torch.randn(*z.shape, generator=g), tdt)
    z.backward(dz)
    oh, ow = z.shape[1:3]
    if isinstance(padding, str):
        pt = OB.same_pads(ih, k[0], stride)[0] if padding == "SAME" else 0
        pl = OB.same_pads(iw, k[1], stride)[0] if padding == "SAME" else 0
    else:
        pt, pl = padding[0], padding[2]
    xld, zld = cin + 8, cout + 16
    xd = torch.zeros(nb, ih, iw, xld, dtype=tdt, device=DEV)
    xd[..., :cin] = x.detach().to(tdt).to(DEV)
    xd[..., cin:] = 3.0                                    # neighbours in the wider buffers must not leak in
    dzd = torch.full((nb, oh, ow, zld), 5.0, dtype=tdt, device=DEV)
    dzd[..., :cout] = dz.to(tdt).to(DEV)
    for cfg in WGRAD_DMA_CFGS:
        dw = torch.full((k[0], k[1], cin, cout), 0.5, device=DEV)
        d = _lib.ConvDesc(nb, ih, iw, cin, xld, k[0], k[1], stride, pt, pl, oh, ow, cout, cout, 0, 0, 0, dt, 0, cfg, 0, 0)
        _lib.check(lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), zld, dw.data_ptr(), st()), "wgrad cfg %d" % cfg)
        close(dw.cpu() - 0.5, w.grad, 3e-5)


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("cfg", [92, 94, 96])
@pytest.mark.parametrize("padding,cout,nb,ih,iw", [("VALID", 32, 3, 37, 43), ("SAME", 64, 2, 35, 66), ("SAME", 32, 2, 109, 109),
                                                   ("VALID", 64, 2, 10, 26), ("SAME", 24, 3, 16, 33), ("SAME", 64, 2, 9, 100)])
def test_wgrad_deep_strip_form(padding, cout, nb, ih, iw, cfg, dt, tdt, eps):
    """tile_cfg 92..96: the strip form of the 32-input-channel 3x3 layers (Conv2d_2a / 2b) with 8 x 32-pixel strips (16
    k-steps per LDS fill instead of 2) — ragged widths and heights (strips that end inside the map), SAME and VALID, 24 /
    32 / 64 output channels, operands that are channel slices of wider buffers: against autograd on the same 16-bit values."""
    g = torch.Generator().manual_seed(cfg * 31 + ih + iw + cout)
    x = q(torch.randn(nb, ih, iw, 32, generator=g), tdt).requires_grad_(True)
    w = q(torch.randn(3, 3, 32, cout, generator=g) * 0.1, tdt).requires_grad_(True)
    z = OB.conv2d(x, w, 1, padding)
    dz = q(torch.randn(*z.shape, generator=g), tdt)
    z.backward(dz)
    oh, ow = z.shape[1:3]
    p = 1 if padding == "SAME" else 0
    xld, zld = 32 + 8, cout + 16
    xd = torch.full((nb, ih, iw, xld), 3.0, dtype=tdt, device=DEV)
    xd[..., :32] = x.detach().to(tdt).to(DEV)
    dzd = torch.full((nb, oh, ow, zld), 5.0, dtype=tdt, device=DEV)
    dzd[..., :cout] = dz.to(tdt).to(DEV)
    dw = torch.full((3, 3, 32, cout), 0.5, device=DEV)
    d = _lib.ConvDesc(nb, ih, iw, 32, xld, 3, 3, 1, p, p, oh, ow, cout, cout, 0, 0, 0, dt, 0, cfg, 0, 0)
    _lib.check(lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), zld, dw.data_ptr(), st()), "wgrad")
    close(dw.cpu() - 0.5, w.grad, 3e-5)


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
def test_batched_filter_packing_equals_the_per_filter_call(dt, tdt, eps):
    """gv_pack_filters_batched: forward and data-gradient (flipped + transposed) images of many filters in one launch,
    bit for bit what gv_pack_filter_hwio makes of W and of flip(W)^T."""
    g = torch.Generator().manual_seed(21)
    shapes = [(3, 3, 32, 48), (1, 7, 48, 32), (5, 5, 48, 64), (1, 1, 96, 40), (7, 1, 128, 192), (3, 3, 3, 32)]
    ws = [torch.randn(*sh, generator=g).to(DEV) for sh in shapes]
    jobs, blocks, outs, refs = [], [], [], []
    for w in ws:
        kh, kw, cin, cout = w.shape
        for flipped in (0, 1):
            if flipped and cin % 8:
                continue
            src = torch.flip(w, (0, 1)).permute(0, 1, 3, 2).contiguous() if flipped else w
            a, b = (cout, cin) if flipped else (cin, cout)
            n = lib().gv_packed_filter_bytes(kh, kw, a, b, dt, 0)
            ref = torch.zeros(n, dtype=torch.uint8, device=DEV)
            _lib.check(lib().gv_pack_filter_hwio(src.data_ptr(), kh, kw, a, b, ref.data_ptr(), dt, 0, st()), "pack")
            out = torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV)
            rows, k = (cin, kh * kw * cout) if flipped else (cout, kh * kw * cin)
            nblk = (rows * ((k + 31) // 32 * 32) + 255) // 256
            jobs.append(_lib.PackJob(w.data_ptr(), out.data_ptr(), kh, kw, cin, cout, flipped, len(blocks)))
            blocks.extend([len(jobs) - 1] * nblk)
            outs.append(out)
            refs.append(ref)
    jd = torch.frombuffer(bytearray(b"".join(bytes(j) for j in jobs)), dtype=torch.uint8).to(DEV)
    bj = torch.tensor(blocks, dtype=torch.int32, device=DEV)
    _lib.check(lib().gv_pack_filters_batched(jd.data_ptr(), len(jobs), bj.data_ptr(), bj.numel(), dt, st()), "batched")
    torch.cuda.synchronize()
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)
    assert lib().gv_pack_filters_batched(jd.data_ptr(), len(jobs), bj.data_ptr(), bj.numel(), _lib.GV_F32, st()) != 0


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("per_shape", [0, 1])
def test_view_pool_fuse_backward_typed(dt, tdt, eps, per_shape):
    g = torch.Generator().manual_seed(3)
    V, N, E, G = 6, 3, 40, 5
    F = q(torch.randn(N, V, E, generator=g), tdt)
    F[:, 1] = F[:, 0]                                    # ties inside a group
    dS = torch.randn(N, E, generator=g)
    sch = torch.zeros(N if per_shape else 1, G, V, dtype=torch.int32)
    for n in range(sch.shape[0]):
        for v in range(V):
            sch[n, (v + n) % 3, v] = 1                   # groups 3, 4 stay empty
    wt = 1.0 + sch.sum(-1).float()
    Fd = F.to(tdt).to(DEV)
    dF = torch.full_like(Fd, 0.5)
    _lib.check(lib().gv_view_pool_fuse_bwd_t(Fd.data_ptr(), dS.to(DEV).data_ptr(), V, N, E, E, V * E,
                                             sch.to(DEV).data_ptr(), G, wt.to(DEV).data_ptr(), _lib.GV_VIEWPOOL_MAX,
                                             dF.data_ptr(), per_shape, dt, st()), "fuse bwd")
    F32 = F.to(DEV)
    dF32 = torch.zeros_like(F32)
    fn = lib().gv_view_pool_fuse_bwd_per_shape if per_shape else lib().gv_view_pool_fuse_bwd
    _lib.check(fn(F32.data_ptr(), dS.to(DEV).data_ptr(), V, N, E, E, V * E, sch.to(DEV).data_ptr(), G,
                  wt.to(DEV).data_ptr(), _lib.GV_VIEWPOOL_MAX, dF32.data_ptr(), st()), "fuse bwd f32")
    close(dF.float().cpu() - 0.5, dF32.cpu(), 4 * eps)


def _tv(bufs, t):
    return torch.as_strided(bufs[t.vbuf], (t.nb, t.h, t.w, t.c), (t.h * t.w * t.ld, t.w * t.ld, t.ld, 1), t.off)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_bf16_engine_op_by_op_against_the_fp32_engine(backbone, size, N, V):
    """Wiring of the bf16 engine (descriptors, offsets into concat buffers, accumulate semantics, typed entry points),
    op by op with TEACHER FORCING: every op of BOTH engines runs on the same tensors (the fp32 step's activations and
    gradients, rounded to bf16) and the outputs are compared, forward and backward.  This isolates each op's own
    arithmetic (bf16 filter rounding, one rounding per stored output) from two effects that belong to bf16 storage
    itself and not to the engine: rounded activations tie more often inside max-pool windows (the gradient moves to
    the first maximum), and a randomly initialised train-mode-BatchNorm network amplifies ANY perturbation by ~9 %
    per layer (measured: 2.5 % at Mixed_5b -> 65 % at Mixed_7c, identically for bf16 storage and for single-pass
    bf16 math on fp32 storage)."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0][:N])
    e32 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    e16 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage="bf16")
    e16.fuse_bn_pool = False                             # (op by op: the fused pool -> BatchNorm pairs are tests/test_gpu_bn_pool.py's)
    e32.forward(x, labels)
    e32.backward()
    e16.forward(x, labels, g_scheme=e32.scheme.cpu().numpy(), g_weight=e32.weight.cpu().numpy())
    e16.backward()                                       # allocates every gradient buffer
    ref_act = [a.to(torch.bfloat16).float() for a in e32.act]
    ref_grad = [g.to(torch.bfloat16).float() if g is not None else None for g in e32.grad]
    x32 = e32._x.to(torch.bfloat16).float()
    e32._x = x32                                         # the network input too
    worst, y_forced = {}, {}

    def note(kind, what, err, name):
        key = (kind, what)
        if err > worst.get(key, (0.0, ""))[0]:
            worst[key] = (err, name)

    def force_act(t):
        if t is not None and t.vbuf >= 0:
            e16.act[t.vbuf].copy_(ref_act[t.vbuf])
            e32.act[t.vbuf].copy_(ref_act[t.vbuf])
    for o32, o16 in zip(e32.plan.ops, e16.plan.ops):
        force_act(o16["x"])
        force_act(o16.get("res"))
        e32._forward_op(o32)
        e16._forward_op(o16)
        note(o16["kind"], "y", _rel(e16.view(o16["y"]).float(), e32.view(o32["y"])), o16["name"])
        y_forced[id(o32)] = e32.view(o32["y"]).to(torch.bfloat16)    # (the output that belongs to the forced input)
    for o32, o16 in zip(reversed(e32.plan.ops), reversed(e16.plan.ops)):
        xt, yt, rt = o32["x"], o32["y"], o32.get("res")
        if yt.vbuf < 0 or ref_grad[yt.vbuf] is None:
            continue
        pnames = [k for k in e32.grads if k.startswith(o32["name"] + "/") or k == o32.get("bias")]
        if o32["kind"] == "conv":
            pnames = [m[0] for m in e32._members(o32)] + ([o32["bias"]] if o32.get("bias") else [])
        for e in (e32, e16):
            if o32.get("members"):
                e._dw(o32 if e is e32 else o16).zero_()
        for e, o in ((e32, o32), (e16, o16)):
            for t in (xt, rt):
                if t is not None and t.vbuf >= 0 and e.grad[t.vbuf] is not None:
                    e.grad[t.vbuf].zero_()
            e.grad[yt.vbuf].copy_(ref_grad[yt.vbuf])
            for k in pnames:
                e.grads[k].zero_()
        for t in (xt, yt, rt):
            force_act(t)
        if o32["kind"] == "bn":                              # its ReLU mask: the forced forward's own output
            e32.view(yt).copy_(y_forced[id(o32)])
            e16.view(yt).copy_(y_forced[id(o32)])
        assert xt.vbuf != yt.vbuf
        e32._backward_op(o32)
        e16._backward_op(o16)
        if xt.vbuf >= 0:
            note(o16["kind"], "dx", _rel(e16.view(xt, grad=True).float(), e32.view(xt, grad=True)), o16["name"])
        if rt is not None:
            note(o16["kind"], "dres", _rel(e16.view(rt, grad=True).float(), e32.view(rt, grad=True)), o16["name"])
        for k in pnames:
            note(o16["kind"], "d" + k.rsplit("/", 1)[1], _rel(e16.grads[k], e32.grads[k]), k)
    torch.cuda.synchronize()
    for key in sorted(worst):
        print("%-5s %-10s worst rel_l2 %.5f  (%s)" % (key[0], key[1], worst[key][0], worst[key][1]))
    for key, (err, name) in worst.items():
        assert err < OP_BOUND, (key, err, name)


OP_BOUND = 0.01
S_BOUND = 0.25


def _flat(grads, names):
    return torch.cat([grads[k].reshape(-1).double().cpu() for k in names])


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_bf16_training_step_tracks_the_fp32_step(backbone, size, N, V):
    """The whole step on bf16 storage beside the fp32 engine (same variables, same batch, same scheme).  A randomly
    initialised network with train-mode BatchNorm amplifies any perturbation by ~9 % per layer (see the op-by-op test:
    single-pass bf16 math on fp32 storage drifts exactly as far), so end to end only coarse agreement is meaningful:
    descriptor within 25 % in norm, loss within 3 %, and a Momentum step on the bf16 gradient lowers the loss."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    shapes = eng.plan.param_shapes()
    P = gv.params.init_backbone_params(shapes, seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0][:N])
    e32 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV)
    _, S32, logits32, loss32 = e32.forward(x, labels)
    S32, logits32, loss32 = S32.clone(), logits32.clone(), loss32.clone()
    g32 = {k: v.clone() for k, v in e32.backward().items()}
    scheme, weight = e32.scheme.cpu().numpy(), e32.weight.cpu().numpy()
    e16 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage="bf16")
    assert e16.act[0].dtype == torch.bfloat16
    _, S16, logits16, loss16 = e16.forward(x, labels, g_scheme=scheme, g_weight=weight)
    S16, logits16 = S16.clone(), logits16.clone()
    g16 = e16.backward()
    torch.cuda.synchronize()
    def rel_l2(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).norm() / b.norm())
    names = sorted(g32)
    a, d = _flat(g16, names), _flat(g32, names)
    cos = float((a @ d) / (a.norm() * d.norm()))
    rel = float((a - d).norm() / d.norm())
    eS, eL = rel_l2(S16.float(), S32), rel_l2(logits16, logits32)
    print("bf16 vs fp32 step: S %.4f, logits %.4f, loss %.5f vs %.5f, gradient cosine %.4f, relative error %.3f"
          % (eS, eL, float(loss16), float(loss32), cos, rel))
    assert eS < S_BOUND and eL < S_BOUND
    assert abs(float(loss16) - float(loss32)) <= 0.03 * max(1.0, abs(float(loss32)))
    assert all(bool(torch.isfinite(v).all()) for v in g16.values())
    # one Momentum step moves the loss down on the same batch
    l0 = float(loss16)                                   # (the engine returns its own loss buffer: read it now)
    e16.apply_momentum(lr=1e-4, mu=0.9, weight_decay=1e-4)
    _, _, _, loss1 = e16.forward(x, labels, g_scheme=scheme, g_weight=weight)
    assert float(loss1) < l0


@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_bf16_step_with_frozen_statistics_tracks_the_fp32_step(backbone, size, N, V):
    """The non-chaotic whole-step check of the bf16 path: with BatchNorm on its moving statistics (frozen_bn=True) the bf16
    engine is held against the fp32-storage engine on the same variables, batch and scheme.  Every stored activation and
    activation gradient is rounded to 8 mantissa bits once (relative 2^-9 = 2e-3 rms-ish per rounding); through ~50 layers
    forward and ~50 backward these add like a random walk: sqrt(100) * 2e-3 = 2e-2, and a few ReLU masks differ.  Bound:
    descriptor / logits 5e-2, total gradient 1e-1 in relative L2 with cosine >= 0.99, every value finite.  Measured
    (Inception / ResNet): descriptor 0.4 % / 1.3 %, logits 0.2 % / 0.7 %, gradient 4.7 % / 7.6 %, cosine 0.9989 / 0.9971 (the
    same comparison on batch statistics: cosine 0.05); the deepest tensors of the backward pass, the stem filters, carry
    the largest share (37-42 %)."""
    C_, G = 5, 10
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    del eng
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0][:N])
    e32 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, frozen_bn=True)
    _, S32, logits32, loss32 = e32.forward(x, labels)
    S32, logits32, loss32 = S32.clone(), logits32.clone(), float(loss32)
    g32 = {k: v.clone() for k, v in e32.backward().items()}
    scheme, weight = e32.scheme.cpu().numpy(), e32.weight.cpu().numpy()
    e16 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage="bf16",
                     frozen_bn=True)
    _, S16, logits16, loss16 = e16.forward(x, labels, g_scheme=scheme, g_weight=weight)
    S16, logits16, loss16 = S16.clone(), logits16.clone(), float(loss16)
    g16 = e16.backward()
    torch.cuda.synchronize()

    def rel_l2(a, b):
        a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
        return float((a - b).norm() / b.norm())
    names = sorted(g32)
    a, d = _flat(g16, names), _flat(g32, names)
    cos = float((a @ d) / (a.norm() * d.norm()))
    rel = float((a - d).norm() / d.norm())
    worst = max((rel_l2(g16[k], g32[k]), k) for k in names if float(g32[k].norm()) > 1e-3 * float(d.norm()))
    print("frozen bf16 vs fp32 step, %s: S %.4f logits %.4f loss %.5f vs %.5f; gradient rel %.4f cos %.5f; worst tensor %.3f (%s)"
          % (backbone, rel_l2(S16.float(), S32), rel_l2(logits16, logits32), loss16, loss32, rel, cos, worst[0], worst[1]))
    assert rel_l2(S16.float(), S32) < 5e-2 and rel_l2(logits16, logits32) < 5e-2
    assert abs(loss16 - loss32) <= 1e-2 * max(1.0, abs(loss32))
    assert all(bool(torch.isfinite(v).all()) for v in g16.values())
    assert rel < 1e-1 and cos > 0.99


def test_bf16_step_at_the_real_c3_geometry_beside_the_fp32_step():
    """configs[2] at its real geometry (12 views x 224 x 224, N = 8) on bf16 storage beside the fp32-storage engine, same
    variables, batch and scheme.  What this CAN hold on a randomly initialised network: train-mode BatchNorm re-normalises
    every layer, so a 2^-8 storage rounding grows by ~9 % per layer and the two forward passes drift apart (measured:
    shape descriptor 32 %, logits 8.5 % in relative L2) — below Mixed_7 the two gradients are then gradients of different
    functions (cosine 0.05; the fp32 ORACLE is as far from an fp64 run of itself at small geometry, see
    test_training_step_against_an_fp64_arbiter).  The well-conditioned quantities are asserted: the loss (3e-4 apart),
    the classifier's gradient and the gradients of the layers that write the final concat (0.7 % / 5 %), finiteness
    everywhere, and descent."""
    backbone, size, N, V, C_, G = "inception_v3", 224, 8, 12, 40, 7
    eng = TrainGVCNN(backbone, N, V, size, size, C_, G, device=DEV, num_bins=G)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C_, seed=3, spread_scores=True)
    del eng
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0, 7, 9, 30, 12])
    e32 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, num_bins=G)
    _, S32, logits32, loss32 = e32.forward(x, labels)
    S32, logits32, loss32 = S32.clone(), logits32.clone(), float(loss32)
    g32 = {k: v.clone() for k, v in e32.backward().items()}
    scheme, weight = e32.scheme.cpu().numpy(), e32.weight.cpu().numpy()
    del e32
    e16 = TrainGVCNN(backbone, N, V, size, size, C_, G, backbone_params=P, head_params=Hd, device=DEV, storage="bf16",
                     num_bins=G)
    _, S16, logits16, loss16 = e16.forward(x, labels, g_scheme=scheme, g_weight=weight)
    S16, logits16, l0 = S16.clone(), logits16.clone(), float(loss16)
    g16 = e16.backward()
    torch.cuda.synchronize()

    def rel_l2(a, b):
        a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
        return float((a - b).norm() / b.norm())
    assert abs(l0 - loss32) <= 5e-3 * abs(loss32)
    assert rel_l2(logits16, logits32) < 0.25 and rel_l2(S16.float(), S32) < 0.6
    assert all(bool(torch.isfinite(v).all()) for v in g16.values())
    assert rel_l2(g16["dense_%d/bias" % V], g32["dense_%d/bias" % V]) < 0.05
    last = ["InceptionV3/Mixed_7c/Branch_0/Conv2d_0a_1x1/BatchNorm/beta",      # layers that write the final concat directly
            "InceptionV3/Mixed_7c/Branch_1/Conv2d_0b_1x3/BatchNorm/beta"]
    errs = {k: rel_l2(g16[k], g32[k]) for k in g32 if k.startswith("InceptionV3/Mixed_7c/") and k.endswith("/beta")}
    print("Mixed_7c beta gradients, bf16 vs fp32:", {k.split("/", 2)[2]: round(v, 3) for k, v in sorted(errs.items())})
    assert max(errs[k] for k in last) < 0.2
    e16.apply_momentum(lr=1e-4, mu=0.9, weight_decay=1e-4)
    _, _, _, loss1 = e16.forward(x, labels, g_scheme=scheme, g_weight=weight)
    assert float(loss1) < l0


@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("backbone,size,N,V", [("inception_v3", 171, 4, 2), ("resnet_v2_50", 97, 3, 2)])
def test_first_writer_stores_equal_zero_fill_and_accumulate(backbone, size, N, V, storage):
    """The 16-bit backward pass keeps no zero-filled gradient buffers: the first contribution to a tensor's gradient
    stores, later ones add, and the ReLU mask is recomputed from z.  Against the plain form (zero-fill everything,
    always accumulate, mask read from y) on the same forward pass the gradients must be IDENTICAL: same addends,
    same order, same masks."""
    eng = TrainGVCNN(backbone, N, V, size, size, 5, 10, device=DEV, storage=storage)
    # (the plain form cannot fold its BatchNorm sums into the data-gradient launches — it takes its masks from y — so
    # the folded sums, equal to the separate ones to summation order only, are switched off on both sides: this test is
    # about WHICH addends reach a gradient buffer, bit for bit)
    eng.fuse_bn_stats = False
    eng.fuse_bn_pool = False                              # (the pool -> BatchNorm pairs never materialise the BN output this test
                                                          # compares buffer by buffer: tests/test_gpu_bn_pool.py covers them)
    eng.alias_residual_grad = False                       # (a ResNet shortcut's gradient otherwise LIVES in dy's buffer, which then
                                                          # holds another tensor's gradient at the end of the pass; that form has
                                                          # its own bit-for-bit test in tests/test_gpu_wgrad_det.py)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0][:N])
    eng.forward(x, labels, check=False)
    assert eng._lazy

    def same(a, b):                                      # fp32 storage: its pool backward scatters with fp32 atomics
        if storage == "bf16":
            return torch.equal(a, b)
        return float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30)

    def run():
        grads = {k: v.clone() for k, v in eng.backward().items()}
        acts = {}
        for op in eng.plan.ops:
            t = op["x"]
            if t.vbuf >= 0 and (t.vbuf, t.off, t.c) in written:
                acts[(t.vbuf, t.off, t.c)] = eng.view(t, grad=True).clone()
        return grads, acts
    eng.backward()
    written = set(eng._written)
    assert len(written) > 50
    lazy = run()
    for g in eng.grad:                                   # poison: nothing may depend on what the buffers held
        if g is not None:
            g.fill_(float("nan"))
    lazy2 = run()
    eng._lazy = False
    plain = run()
    torch.cuda.synchronize()
    for k in plain[1]:                                   # activation gradients: bit for bit
        assert bool(torch.isfinite(lazy2[1][k].float()).all()), k
        assert same(lazy[1][k], lazy2[1][k]), k
        assert same(lazy[1][k], plain[1][k]), k
    big = max(float(v.abs().max()) for v in plain[0].values())
    for k in plain[0]:                                   # variables: fp32 atomics in the filter gradient, order varies
        assert float((lazy2[0][k] - plain[0][k]).abs().max()) <= 1e-4 * max(float(plain[0][k].abs().max()), 1e-3 * big), k


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_stream_lanes_reproduce_the_single_stream_step(storage):
    """enable_lanes(): the branches of an Inception block on separate streams, ordered by per-tensor events.  Same
    kernels, same operands: activations and activation gradients are bit-identical to the single-stream step.  (Capturing
    the multi-stream step into one graph is NOT covered: hipStreamEndCapture crashes on it in this runtime, see
    tools/lanes_capture_probe.py; the single-stream step captures fine.)"""
    N, V, size = 4, 3, 171
    eng = TrainGVCNN("inception_v3", N, V, size, size, 5, 10, device=DEV, storage=storage)
    eng.fuse_bn_pool = False                              # (every activation buffer is compared: see tests/test_gpu_bn_pool.py)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2, 0]).to(DEV)

    def snapshot():
        torch.cuda.synchronize()
        return ([a.clone() for a in eng.act], [g.clone() if g is not None else None for g in eng.grad],
                float(eng.loss), eng._flat_g.clone())
    eng.forward(x, labels, check=False)
    eng.backward()
    ref = snapshot()
    lanes_used = {op["lane"] for op in eng.plan.ops}
    assert lanes_used == {0, 1, 2}
    eng.enable_lanes()
    for a in eng.act:
        a.fill_(float("nan"))
    eng.forward(x, labels, check=False)
    eng.backward()
    got = snapshot()
    # the parameter gradients too: the deterministic filter gradient stages its slices in a workspace PER LANE (a shared
    # one would let one lane's slice stores overwrite what another lane's reduce is still reading); bf16 storage: every
    # backward kernel is deterministic, so the whole gradient arena is the same bits
    if storage == "bf16":
        assert torch.equal(got[3], ref[3])
    else:
        assert float((got[3] - ref[3]).abs().max()) <= 1e-5 * float(ref[3].abs().max())
    for other in (got,):
        assert other[2] == ref[2]
        for a, b in zip(other[0], ref[0]):
            assert torch.equal(a, b)
        for a, b in zip(other[1], ref[1]):
            if b is not None:
                if storage == "bf16":                    # (unwritten regions keep whatever they held)
                    mask = ~torch.isnan(b.float())
                    assert torch.equal(a[mask], b[mask])
                else:                                    # (its pool backward scatters with fp32 atomics)
                    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.parametrize("backbone,storage,size", [("inception_v3", "bf16", 171), ("resnet_v2_50", "bf16", 96), ("inception_v3", "f32", 139)])
def test_recorded_argmax_pools_reproduce_the_recomputing_step(backbone, storage, size):
    """TrainGVCNN.pool_argmax (the max pools record their winners in the forward pass, the backward pass routes dy by the
    record) against the form that recomputes the winners from x: the same loss, activations and (16-bit storage: both
    backward forms are deterministic gathers of the same values) activation gradients bit for bit, the same parameter
    gradients to the rounding of their atomic sums."""
    N, V = 3, 2
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(7)) - 0.5).to(DEV)
    labels = torch.tensor([1, 4, 2]).to(DEV)
    out = []
    for amax in (True, False):
        eng = TrainGVCNN(backbone, N, V, size, size, 5, 10, device=DEV, storage=storage, seed=5)
        eng.pool_argmax = amax
        eng.fuse_bn_pool = False                         # (the pool -> BatchNorm pairs need the record: tests/test_gpu_bn_pool.py)
        eng.forward(x, labels, check=False)
        eng.backward()
        torch.cuda.synchronize()
        assert any("argmax" in op for op in eng.plan.ops) == amax
        out.append((float(eng.loss), eng._flat_g.clone(), [a.clone() for a in eng.act],
                    [g.clone() if g is not None else None for g in eng.grad]))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][2], out[1][2]):
        assert torch.equal(a, b)
    if storage == "bf16":                                 # activation gradients: the same values gathered in the same order
        for a, b in zip(out[0][3], out[1][3]):
            if b is not None:
                mask = ~torch.isnan(b.float())            # (unwritten regions keep whatever they held)
                assert torch.equal(a[mask], b[mask])
    # parameter gradients: the filter gradient adds its pixel slices with fp32 atomics, so two runs agree to rounding only
    assert float((out[0][1] - out[1][1]).abs().max()) <= 2e-5 * float(out[1][1].abs().max())


def test_bf16_training_autotune_and_per_shape_step_runs():
    eng = TrainGVCNN("inception_v3", 2, 3, 139, 139, 10, 10, device=DEV, storage="bf16", per_shape=True)
    x = (torch.rand(2, 3, 139, 139, 3, generator=torch.Generator().manual_seed(4)) - 0.5).to(DEV)
    labels = torch.tensor([3, 7])
    eng.forward(x, labels, check=False)
    eng.autotune(iters=1)
    l0 = float(eng.train_step(x, labels, lr=1e-4))
    assert np.isfinite(l0)
    for _ in range(3):
        l1 = float(eng.train_step(x, labels, lr=1e-4))
    assert np.isfinite(l1) and l1 < l0


@pytest.mark.parametrize("backbone,storage,N,V,size,kw", [("inception_v3", "bf16", 2, 20, 299, {}),
                                                         ("inception_v3", "f16", 2, 3, 171, {}),
                                                         ("resnet_v2_50", "bf16", 3, 4, 129, {"per_shape": True})])
def test_16bit_training_runs_at_other_geometries(backbone, storage, N, V, size, kw):
    """configs[4]'s geometry (20 views, 299x299) on the bf16 step, the fp16 instantiation of the engine, ResNet with
    per-shape grouping: a few steps on one batch lower the loss, every gradient stays finite."""
    eng = TrainGVCNN(backbone, N, V, size, size, 10, 10, device=DEV, storage=storage, **kw)
    x = (torch.rand(N, V, size, size, 3, generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV)
    y = torch.randint(0, 10, (N,), generator=torch.Generator().manual_seed(1)).to(DEV)
    losses = [float(eng.train_step(x, y, lr=3e-4)) for _ in range(4)]
    grads = eng.backward()
    assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())


# ---- stride-2 data gradient by parity classes (gv_conv_desc.y_step) -----------------------------------------------------
S2_CONVS = [((3, 3), (0, 0), 288, 384, 3, 25, 25),       # Mixed_6a/Branch_0 (nets/inception_v3.py:210): 25 -> 12, VALID
            ((3, 3), (0, 0), 96, 96, 4, 12, 13),         # odd and even maps, rows no window reaches
            ((3, 3), (1, 1), 64, 64, 3, 14, 14),         # ResNet conv2 of a stride-2 unit: pad(1,1) + VALID
            ((3, 3), (0, 0), 192, 320, 5, 4, 4)]         # a 4x4 map (Mixed_7a at a 96-pixel input): 1x1 output


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("k,pads,cin,cout,nb,ih,iw", S2_CONVS)
def test_stride2_data_gradient_by_parity_classes(dt, tdt, eps, k, pads, cin, cout, nb, ih, iw):
    """dX of a stride-2 convolution as FOUR stride-1 launches over the un-dilated dZ, one per (row parity, column parity)
    of dX, each with the taps that reach that parity and a two-level output stride — against torch autograd through the
    oracle's convolution (the zero-dilated single launch is held to the same reference above), in store and in
    accumulate mode, filters packed by gv_pack_filters_batched's sub_step form straight from the HWIO variable."""
    g = torch.Generator().manual_seed(5)
    x = q(torch.randn(nb, ih, iw, cin, generator=g), tdt).requires_grad_(True)
    w = q(torch.randn(k[0], k[1], cin, cout, generator=g) * 0.1, tdt).requires_grad_(True)
    z = OB.conv2d(x, w, 2, (pads[0], pads[0], pads[1], pads[1]))
    dz = q(torch.randn(*z.shape, generator=g), tdt)
    z.backward(dz)
    oh, ow = z.shape[1:3]
    xld, zld = cin + 8, cout + 16
    dzd = torch.zeros(nb, oh, ow, zld, dtype=tdt, device=DEV)
    dzd[..., :cout] = dz.to(tdt).to(DEV)
    wd = w.detach().to(DEV).contiguous()
    classes, jobs, blocks = [], [], []
    for py in (0, 1):
        for px in (0, 1):
            r0, s0 = (py + pads[0]) % 2, (px + pads[1]) % 2
            th, tw = len(range(r0, k[0], 2)), len(range(s0, k[1], 2))
            pt, pl = (th - 1) - (py + pads[0] - r0) // 2, (tw - 1) - (px + pads[1] - s0) // 2
            A, B = len(range(py, ih, 2)), len(range(px, iw, 2))
            assert th >= 1 and tw >= 1 and pt >= 0 and pl >= 0
            buf = torch.zeros(lib().gv_packed_filter_bytes(th, tw, cout, cin, dt, 0), dtype=torch.uint8, device=DEV)
            kc = th * tw * cout
            jobs.append(_lib.PackJob(wd.data_ptr(), buf.data_ptr(), th, tw, cin, cout, 1, len(blocks), 0, 0, 0, 2, r0, s0, k[1]))
            blocks.extend([len(jobs) - 1] * ((cin * ((kc + 31) // 32 * 32) + 255) // 256))
            classes.append((py, px, th, tw, pt, pl, A, B, buf))
    jd = torch.frombuffer(bytearray(b"".join(bytes(j) for j in jobs)), dtype=torch.uint8).to(DEV)
    bj = torch.tensor(blocks, dtype=torch.int32, device=DEV)
    _lib.check(lib().gv_pack_filters_batched(jd.data_ptr(), len(jobs), bj.data_ptr(), bj.numel(), dt, st()), "pack")
    ones, zeros = torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV)
    for accumulate in (0, 1):
        dx = torch.full((nb, ih, iw, xld), 0.25, dtype=tdt, device=DEV)
        for tile in (0, 2, 14):
            dx.fill_(0.25)
            for py, px, th, tw, pt, pl, A, B, buf in classes:
                d = _lib.ConvDesc(nb, oh, ow, cout, zld, th, tw, 1, pt, pl, A, B, cin, xld, xld if accumulate else 0, 0, 0, dt,
                                  0, tile, 0, 0, 0, 2, py, px, ih, iw)
                _lib.check(lib().gv_conv2d_fwd(C.byref(d), dzd.data_ptr(), buf.data_ptr(), ones.data_ptr(), zeros.data_ptr(),
                                               dx.data_ptr() if accumulate else None, dx.data_ptr(), None, None, None, st()),
                           "parity class (%d, %d)" % (py, px))
            got = dx[..., :cin].float().cpu() - (0.25 if accumulate else 0.0)
            close(got, x.grad, 2 * eps)
            assert float((dx[..., cin:].float() - 0.25).abs().max()) == 0.0     # the wider buffer's other channels untouched


def test_wgrad_on_one_pixel_wide_maps():
    """1-wide / 1-high output maps (the last blocks at small inputs): the LDS-DMA filter gradient's pixel walk divides by
    the map size with a 32-bit reciprocal that does not exist for 1 — those layers must take the other tiles (advisor
    finding of round 2: every pixel past the first 32 of a workgroup's slice was dropped)."""
    dt, tdt = _lib.GV_BF16, torch.bfloat16
    g = torch.Generator().manual_seed(3)
    for (ih, iw, kh, kw, pt, pl) in ((1, 1, 1, 1, 0, 0), (1, 5, 1, 3, 0, 1), (7, 1, 3, 1, 1, 0)):
        nb, cin, cout = 80, 64, 96                          # 80 images: more than 32 pixels per workgroup slice
        x = q(torch.randn(nb, ih, iw, cin, generator=g), tdt).requires_grad_(True)
        w = q(torch.randn(kh, kw, cin, cout, generator=g) * 0.1, tdt).requires_grad_(True)
        z = OB.conv2d(x, w, 1, (pt, pt, pl, pl))
        dz = q(torch.randn(*z.shape, generator=g), tdt)
        z.backward(dz)
        xd, dzd = x.detach().to(tdt).to(DEV), dz.to(tdt).to(DEV)
        for cfg in (0, 1, 31, 43, 47):
            dw = torch.zeros(kh, kw, cin, cout, device=DEV)
            d = _lib.ConvDesc(nb, ih, iw, cin, cin, kh, kw, 1, pt, pl, ih, iw, cout, cout, 0, 0, 0, dt, 0, cfg, 0, 0)
            rc = lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), cout, dw.data_ptr(), st())
            if rc == _lib.GV_E_UNSUPPORTED and cfg >= 31:
                continue                                    # the LDS-DMA forms decline 1-wide maps
            _lib.check(rc, "wgrad cfg %d" % cfg)
            close(dw.cpu(), w.grad, 3e-5)


@pytest.mark.parametrize("dt,tdt,eps", TYPES)
@pytest.mark.parametrize("k,pad,cout,nb,ih,iw", [(3, 0, 32, 37, 23, 40), (3, 0, 64, 9, 47, 72), (7, 2, 64, 5, 33, 48),
                                                 (3, 0, 32, 3, 224, 224), (7, 3, 64, 3, 224, 224), (7, 3, 64, 2, 200, 216), (7, 3, 64, 5, 33, 48)])
def test_stem_filter_gradient_on_row_strips(dt, tdt, eps, k, pad, cout, nb, ih, iw):
    """The 3-channel stems' filter gradient (Conv2d_1a 3x3/2, nets/inception_v3.py:97; a 7x7/2 with padding) on
    conv_wgrad_stem_rows_lp — image rows and the dZ row through LDS, 16-bit MFMA — against torch autograd through the
    oracle's convolution; products of 16-bit values are exact in fp32, so only the summation order differs."""
    g = torch.Generator().manual_seed(k * 100 + cout)
    x = q(torch.rand(nb, ih, iw, 3, generator=g) - 0.5, tdt).requires_grad_(True)
    w = q(torch.randn(k, k, 3, cout, generator=g) * 0.2, tdt).requires_grad_(True)
    big = nb * ih * iw > 100000
    dev = DEV if big else "cpu"
    z = OB.conv2d(x.to(dev), w.to(dev), 2, (pad, pad, pad, pad))
    dz = q(torch.randn(*z.shape, generator=g), tdt)
    z.backward(dz.to(z.device))
    oh, ow = z.shape[1:3]
    zld = cout + 16
    xd = x.detach().to(tdt).to(DEV).contiguous()
    dzd = torch.zeros(nb, oh, ow, zld, dtype=tdt, device=DEV)
    dzd[..., :cout] = dz.to(tdt).to(DEV)
    outs = []
    for f32 in (0, 1):                                   # the new kernel, then the fp32-MFMA direct kernel it replaces
        lib().gv_conv2d_wgrad_set_lp_f32(f32)
        dw = torch.full((k, k, 3, cout), 0.5, device=DEV)
        d = _lib.ConvDesc(nb, ih, iw, 3, 3, k, k, 2, pad, pad, oh, ow, cout, cout, 0, 0, 0, dt, 0, 0, 0, 0)
        _lib.check(lib().gv_conv2d_wgrad(C.byref(d), xd.data_ptr(), dzd.data_ptr(), zld, dw.data_ptr(), st()), "wgrad")
        outs.append(dw.cpu() - 0.5)
    lib().gv_conv2d_wgrad_set_lp_f32(0)
    close(outs[0], w.grad.cpu(), 5e-5 if not big else 3e-4)
    close(outs[0], outs[1], 5e-5 if not big else 3e-4)
