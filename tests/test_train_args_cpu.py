"""Argument codes of the training step's HBM-bound ops (csrc/train.hip): the BatchNorm sums and apply, the ReLU/BatchNorm
backward, accumulate, the bias gradient and the view-pool backward, each in its fp32 form and its storage-typed `_t` form.
Every call in the table is rejected before any HIP call, so this runs without a device; the codes are literals."""
import pytest
import torch                                       # noqa: F401  (before the library, as in the GPU test files)

from gvcnn_tf_amd import _lib

P = 4096                                           # a 16-byte aligned stand-in address: never dereferenced
F32, BF16, F16 = _lib.GV_F32, _lib.GV_BF16, _lib.GV_F16
ZEROED, RAW_Z = _lib.GV_ACCUM_ZEROED, _lib.GV_ACCUM_RAW_Z
BADARG, UNSUPPORTED, ALIGN = -1, -2, -3

# name -> (the arguments of the fp32 form in order with values that pass every check, the arguments `_t` adds)
OPS = {
    "gv_bn_sums_grouped": (dict(z=P, nb=6, hw=35, c=8, z_ld=8, G=3, accum=P), dict()),
    "gv_scale_shift_act_grouped": (dict(x=P, nb=6, hw=35, c=8, x_ld=8, scale=P, shift=P, G=3, relu=1, y=P, y_ld=8), dict()),
    "gv_bn_relu_bwd_sums_grouped": (dict(dy=P, dy_ld=8, y=P, y_ld=8, z=P, z_ld=8, mean=P, inv=P, nb=6, hw=35, c=8, G=3,
                                         accum=P), dict(scale=None, shift=None)),
    "gv_bn_relu_bwd_apply_grouped": (dict(dy=P, dy_ld=8, y=P, y_ld=8, z=P, z_ld=8, mean=P, inv=P, gamma=P, counts=P, nb=6,
                                          hw=35, c=8, G=3, accum=P, dz=P, dz_ld=8, dbeta=P, dgamma=P),
                                     dict(scale=None, shift=None, accumulate=1)),
    "gv_accumulate": (dict(src=P, src_ld=8, dst=P, dst_ld=8, npix=210, c=8), dict()),
    "gv_bias_grad": (dict(dz=P, dz_ld=8, npix=210, c=8, accum=P, dbias=P), dict()),
    "gv_view_pool_fuse_bwd": (dict(F=P, dS=P, V=4, N=2, E=100, vs=100, ss=400, scheme=P, G=3, weight=P, mode=0, dF=P),
                              dict(per_shape=0)),
}


def nulls(*names):
    return [({n: None}, BADARG) for n in names]


# name -> [(arguments that differ from the passing ones, code)]: the rejections both forms share, whatever the dtype
SHARED = {
    "gv_bn_sums_grouped": nulls("z", "accum") + [(dict(nb=7), BADARG), (dict(G=4), BADARG), (dict(z_ld=7), BADARG),
                                                   (dict(nb=0), BADARG), (dict(G=0), BADARG)],
    "gv_scale_shift_act_grouped": nulls("x", "y", "scale", "shift") + [(dict(x_ld=7), BADARG), (dict(y_ld=7), BADARG),
                                                                       (dict(hw=0), BADARG), (dict(G=0), BADARG)],
    "gv_bn_relu_bwd_sums_grouped": nulls("dy", "z", "mean", "inv", "accum") + [(dict(nb=7), BADARG), (dict(G=4), BADARG),
                                                                               (dict(c=0), BADARG)],
    "gv_bn_relu_bwd_apply_grouped": nulls("dy", "z", "mean", "inv", "counts", "accum", "dz") + [
        (dict(nb=7), BADARG), (dict(G=4), BADARG), (dict(hw=0), BADARG)],
    "gv_accumulate": nulls("src", "dst") + [(dict(src_ld=7), BADARG), (dict(dst_ld=7), BADARG), (dict(npix=0), BADARG)],
    "gv_bias_grad": nulls("dz", "accum", "dbias") + [(dict(dz_ld=7), BADARG), (dict(npix=2 ** 31), BADARG),
                                                      (dict(npix=0), BADARG)],
    "gv_view_pool_fuse_bwd": nulls("F", "dS", "scheme", "weight", "dF") + [
        (dict(V=0), BADARG), (dict(E=0), BADARG), (dict(V=65), UNSUPPORTED), (dict(G=65), UNSUPPORTED),
        (dict(N=65536), UNSUPPORTED), (dict(V=65, F=None), BADARG)],
}
# fp32 storage only (both forms): the scalar fp32 kernel works in float4, the 16-bit one takes any shape
F32_ONLY = {
    "gv_scale_shift_act_grouped": [(dict(c=6), ALIGN), (dict(x_ld=9), ALIGN), (dict(y_ld=10), ALIGN), (dict(x=P + 4), ALIGN),
                                   (dict(y=P + 8), ALIGN), (dict(scale=P + 4), ALIGN), (dict(shift=P + 12), ALIGN),
                                   (dict(c=6, x=None), BADARG)],
}
ONE_OF_TWO = [dict(scale=P), dict(shift=P)]        # scale / shift: both or neither
# `_t` form only: (arguments that differ, dtype, code)
TYPED = {
    # the dtype is looked at before the pointers; GV_ACCUM_RAW_Z is no bit of this op
    "gv_bn_sums_grouped": [(dict(z=None), 3, UNSUPPORTED), (dict(nb=7), 7 | ZEROED, UNSUPPORTED),
                           (dict(z=None), F32 | ZEROED, BADARG), (dict(z_ld=7), BF16 | ZEROED, BADARG),
                           (dict(accum=None), F16 | ZEROED, BADARG), (dict(), BF16 | RAW_Z, UNSUPPORTED)],
    "gv_scale_shift_act_grouped": [(dict(x=None), 3, UNSUPPORTED), (dict(), BF16 | ZEROED, UNSUPPORTED)],
    # scale / shift are looked at before the dtype, the dtype before the pointers
    "gv_bn_relu_bwd_sums_grouped": [(a, t, BADARG) for a in ONE_OF_TWO for t in (F32, BF16, F16, 3, BF16 | ZEROED, F32 | RAW_Z)] + [
        (dict(dy=None), 3, UNSUPPORTED), (dict(dy=None, scale=P, shift=P), F16 | ZEROED, BADARG),
        (dict(nb=7), F32 | ZEROED, BADARG), (dict(), BF16 | RAW_Z, UNSUPPORTED)],
    # fp32 storage has no raw-z accumulators; GV_ACCUM_ZEROED is no bit of this op
    "gv_bn_relu_bwd_apply_grouped": [(a, t, BADARG) for a in ONE_OF_TWO for t in (F32, BF16, F16, 3, BF16 | RAW_Z, F32 | RAW_Z)] + [
        (dict(), F32 | RAW_Z, UNSUPPORTED), (dict(dy=None), F32 | RAW_Z, UNSUPPORTED),
        (dict(scale=P, shift=P), F32 | RAW_Z, UNSUPPORTED), (dict(dy=None), 3, UNSUPPORTED),
        (dict(dz=None), BF16 | RAW_Z, BADARG), (dict(nb=7), F16 | RAW_Z, BADARG), (dict(), BF16 | ZEROED, UNSUPPORTED)],
    "gv_accumulate": [(dict(src=None), 3, UNSUPPORTED), (dict(), BF16 | ZEROED, UNSUPPORTED)],
    "gv_bias_grad": [(dict(npix=2 ** 31), 3, UNSUPPORTED), (dict(), F16 | ZEROED, UNSUPPORTED)],
    "gv_view_pool_fuse_bwd": [(dict(F=None), 3, UNSUPPORTED), (dict(V=65), F16, UNSUPPORTED),
                              (dict(G=65, per_shape=1), BF16, UNSUPPORTED), (dict(dF=None, per_shape=1), F32, BADARG)],
}
UNKNOWN_DTYPES = (3, -1, 255, F32 | RAW_Z | ZEROED, 0x400)


def call(lib, fn, base, extra, change, dtype=None):
    a = dict(base)
    if dtype is not None:
        a.update(extra)
    assert set(change) <= set(a), (fn, change)
    a.update(change)
    args = list(a.values()) + ([dtype] if dtype is not None else []) + [None]    # (stream)
    return getattr(lib, fn)(*args)


@pytest.mark.parametrize("name", sorted(OPS))
def test_train_op_argument_codes(name):
    lib = _lib.load()
    base, extra = OPS[name]
    fp32_forms = [name] + (["gv_view_pool_fuse_bwd_per_shape"] if name == "gv_view_pool_fuse_bwd" else [])
    for change, code in SHARED[name] + F32_ONLY.get(name, []):
        for fn in fp32_forms:
            assert call(lib, fn, base, extra, change) == code, (fn, change)
        assert call(lib, name + "_t", base, extra, change, F32) == code, (name, change, "GV_F32")
    for change, code in SHARED[name]:
        for dtype in (BF16, F16):
            assert call(lib, name + "_t", base, extra, change, dtype) == code, (name, change, dtype)
    for dtype in UNKNOWN_DTYPES:
        assert call(lib, name + "_t", base, extra, {}, dtype) == UNSUPPORTED, (name, dtype)
    for change, dtype, code in TYPED[name]:
        assert call(lib, name + "_t", base, extra, change, dtype) == code, (name, change, dtype)
