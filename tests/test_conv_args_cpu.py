"""Argument codes of the convolution entry points (csrc/conv_igemm.hip): gv_conv2d_fwd, gv_conv2d_fwd_xpre and
gv_conv2d_fwd_bnstats.  Every call in the table is rejected before any HIP call, so this runs without a device; the codes
are literals.  Where two conditions fail in one call, the code says which check comes first."""
import ctypes as C

import torch                                       # noqa: F401  (before the library, as in the GPU test files)

from gvcnn_tf_amd import _lib

P = 4096                                           # a 16-byte aligned stand-in address: never dereferenced
F32, BF16, F16 = _lib.GV_F32, _lib.GV_BF16, _lib.GV_F16
X3 = _lib.GV_MATH_BF16X3
RELU, RELU2, SPLIT, X_F32 = _lib.GV_CONV_RELU, _lib.GV_CONV_RELU2, _lib.GV_CONV_SPLIT, _lib.GV_CONV_X_F32
X_P3, Y_P3, Y2_P3 = _lib.GV_CONV_X_P3, _lib.GV_CONV_Y_P3, _lib.GV_CONV_Y2_P3
POOL, POOL_SAME, POOL_ACT2 = _lib.GV_CONV_MAXPOOL3S2, _lib.GV_CONV_MAXPOOL3S2_SAME, _lib.GV_CONV_POOL_ACT2
FWD, BWD = _lib.GV_BN_STATS_FWD, _lib.GV_BN_STATS_BWD
BADARG, UNSUPPORTED, ALIGN = -1, -2, -3

# a 3x3 SAME 32 -> 64 layer on an 8x8 map, 16-bit storage; every row below changes it until a check rejects it
DESC = dict(nb=2, ih=8, iw=8, cin=32, x_ld=32, kh=3, kw=3, stride=1, pad_t=1, pad_l=1, oh=8, ow=8, cout=64, y_ld=64, res_ld=0,
            y2_ld=0, flags=0, dtype=BF16, split_col=0, tile_cfg=0, math_mode=0, in_dilation=0, relu_cols=0, y_step=0, y_py=0,
            y_px=0, y_ih=0, y_iw=0)
ARGS = dict(x=P, xscale=P, xshift=P, w=P, scale=P, shift=P, residual=None, y=P, y2=None, scale2=None, shift2=None)
ENTRY = {"fwd": ("gv_conv2d_fwd", ["x", "w", "scale", "shift", "residual", "y", "y2", "scale2", "shift2"]),
         "xpre": ("gv_conv2d_fwd_xpre", ["x", "xscale", "xshift", "w", "scale", "shift", "residual", "y", "y2", "scale2", "shift2"]),
         "stats": ("gv_conv2d_fwd_bnstats", ["x", "w", "scale", "shift", "residual", "y", "stats"])}
STATS = dict(mode=FWD, groups=2, nseg=1)
SEG = dict(c0=0, c1=64, z_ld=0, z=None, scale=None, shift=None, acc=P)

FP32 = dict(dtype=F32)                              # exact fp32 (12 tiles)
PLANES = dict(dtype=F32, math_mode=X3)              # fp32 storage as three bf16 planes (14 tiles)
XP3 = dict(dtype=F32, math_mode=X3, flags=X_P3)     # ... read from three-plane input (24 tiles)
SPLIT32 = dict(flags=SPLIT, split_col=32, y_ld=32, y2_ld=32)
Y2 = dict(y2=P, scale2=P, shift2=P)
BAD_W = dict(w=P + 4)                               # GV_E_ALIGN from the last check before ConvArgs is filled: shows that
                                                    # everything in front of it passed
ONE_ONE = dict(kh=1, kw=1, pad_t=0, pad_l=0)
BWD_SEG = dict(z=P, z_ld=64)


def desc(*changes, **more):
    d = {}
    for c in changes:
        d.update(c)
    d.update(more)
    return d


def flags(base, f):
    return desc(base, flags=base.get("flags", 0) | f)


# (entry point, descriptor fields that differ, arguments that differ, code[, sums request, its first segment])
CASES = [
    # null pointers and non-positive sizes
    ("fwd", None, {}, BADARG),
] + [("fwd", {}, {n: None}, BADARG) for n in ("x", "w", "scale", "shift", "y")] + [
    ("xpre", {}, dict(xscale=None), BADARG), ("xpre", {}, dict(xshift=None), BADARG), ("xpre", None, dict(xscale=None), BADARG),
    ("stats", {}, {}, BADARG, None), ("stats", None, {}, BADARG),
] + [("fwd", {n: 0}, {}, BADARG) for n in ("nb", "ih", "iw", "cin", "cout", "kh", "kw", "stride", "oh", "ow")] + [
    ("fwd", dict(pad_t=-1), {}, BADARG), ("fwd", dict(pad_l=-1), {}, BADARG), ("fwd", dict(nb=0, dtype=7), {}, BADARG),
    # leading dimensions; split with and without y2
    ("fwd", dict(y_ld=63), {}, BADARG), ("fwd", dict(x_ld=31), {}, BADARG),
    ("fwd", dict(res_ld=63), dict(residual=P), BADARG),
    ("fwd", dict(y2_ld=64), dict(y2=P), BADARG), ("fwd", dict(y2_ld=64), dict(y2=P, scale2=P), BADARG),
    ("fwd", dict(y2_ld=63), Y2, BADARG),
    ("fwd", SPLIT32, {}, BADARG), ("fwd", desc(SPLIT32, split_col=0), dict(y2=P), BADARG),
    ("fwd", desc(SPLIT32, split_col=64), dict(y2=P), BADARG), ("fwd", desc(SPLIT32, y_ld=31), dict(y2=P), BADARG),
    ("fwd", desc(SPLIT32, y2_ld=31), dict(y2=P), BADARG), ("fwd", desc(SPLIT32, x_ld=31), dict(y2=P), BADARG),
    ("fwd", desc(SPLIT32, dtype=7), dict(y2=P), UNSUPPORTED),
    # the window of the last output starts inside the padded input, except for a data gradient
    ("fwd", dict(oh=10), BAD_W, BADARG), ("fwd", dict(ow=10), BAD_W, BADARG), ("fwd", dict(oh=10, dtype=7), {}, BADARG),
    ("fwd", dict(oh=10, in_dilation=2), BAD_W, ALIGN), ("fwd", dict(ow=10, y_step=2), BAD_W, ALIGN),
    ("fwd", dict(oh=10, in_dilation=1), BAD_W, BADARG),
    # dtype, math mode, GV_CONV_X_F32
    ("fwd", dict(dtype=7), {}, UNSUPPORTED), ("fwd", dict(dtype=7, flags=X_F32), {}, UNSUPPORTED),
    ("fwd", desc(FP32, math_mode=9), {}, BADARG), ("fwd", desc(FP32, math_mode=-1), {}, BADARG),
    ("fwd", dict(math_mode=9), BAD_W, ALIGN),                        # (16-bit storage has one math mode: not looked at)
    ("fwd", flags(FP32, X_F32), {}, BADARG), ("fwd", flags(PLANES, X_F32), {}, BADARG),
    ("fwd", desc(FP32, math_mode=9, flags=X_F32), {}, BADARG),
    # the three-plane flags
    ("fwd", dict(flags=X_P3), {}, BADARG), ("fwd", dict(flags=Y_P3), {}, BADARG), ("fwd", flags(FP32, X_P3), {}, BADARG),
    ("fwd", desc(PLANES, math_mode=_lib.GV_MATH_BF16X2, flags=Y_P3), {}, BADARG), ("fwd", flags(PLANES, Y2_P3), {}, BADARG),
    ("fwd", desc(PLANES, flags=Y_P3, cout=60), {}, UNSUPPORTED), ("fwd", desc(PLANES, flags=Y_P3, y2_ld=64), Y2, UNSUPPORTED),
    ("fwd", desc(PLANES, flags=Y_P3, res_ld=66), dict(residual=P), UNSUPPORTED),
    ("fwd", desc(PLANES, flags=Y_P3, y_ld=72), {}, UNSUPPORTED), ("fwd", desc(PLANES, flags=Y_P3, cout=56, y_ld=64), {}, UNSUPPORTED),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y_P3, split_col=24, y2_ld=40), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y2_P3, y2_ld=40), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y2_P3, split_col=40, y_ld=40), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y2_P3, y_ld=34), dict(y2=P), ALIGN),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y2_P3), dict(y2=P, y=P + 4), ALIGN),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y_P3, y2_ld=34), dict(y2=P), ALIGN),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y_P3), dict(y2=P + 8), ALIGN),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y_P3, y2_ld=34, tile_cfg=99), dict(y2=P), ALIGN),
    ("fwd", desc(PLANES, SPLIT32, flags=SPLIT | Y_P3, cout=72, split_col=16, y_ld=16, y2_ld=58), dict(y2=P), ALIGN),
    # tile_cfg: 0 = the default pick, 1 ... table size = an index; checked before the packed filter's alignment
    ("fwd", dict(tile_cfg=-1), {}, BADARG),
    ("fwd", dict(tile_cfg=49), BAD_W, ALIGN), ("fwd", dict(tile_cfg=50), BAD_W, BADARG),
    ("fwd", desc(dtype=F16, tile_cfg=49), BAD_W, ALIGN), ("fwd", desc(dtype=F16, tile_cfg=50), BAD_W, BADARG),
    ("fwd", desc(XP3, tile_cfg=24), BAD_W, ALIGN), ("fwd", desc(XP3, tile_cfg=25), BAD_W, BADARG),
    ("fwd", desc(PLANES, tile_cfg=14), BAD_W, ALIGN), ("fwd", desc(PLANES, tile_cfg=15), BAD_W, BADARG),
    ("fwd", desc(PLANES, math_mode=_lib.GV_MATH_BF16X1, tile_cfg=14), BAD_W, ALIGN),
    ("fwd", desc(PLANES, math_mode=_lib.GV_MATH_BF16X1, tile_cfg=15), BAD_W, BADARG),
    ("fwd", desc(FP32, tile_cfg=12), BAD_W, ALIGN), ("fwd", desc(FP32, tile_cfg=13), BAD_W, BADARG),
    # 31-bit pixel counts, the packed filter's alignment, relu_cols
    ("fwd", dict(nb=65536, ih=256, iw=256, oh=256, ow=256), {}, UNSUPPORTED),
    ("fwd", dict(nb=65536, ih=256, iw=256, oh=256, ow=256), BAD_W, UNSUPPORTED), ("fwd", {}, BAD_W, ALIGN),
    ("fwd", dict(relu_cols=-1), {}, BADARG), ("fwd", dict(relu_cols=-1), BAD_W, ALIGN),
    # in_dilation and y_step
    ("fwd", dict(in_dilation=3), {}, BADARG), ("fwd", dict(in_dilation=-1), {}, BADARG),
    ("fwd", desc(FP32, in_dilation=2), {}, UNSUPPORTED), ("fwd", dict(in_dilation=2, cin=40, x_ld=40), {}, UNSUPPORTED),
    ("fwd", dict(in_dilation=2, stride=2), {}, UNSUPPORTED), ("fwd", dict(in_dilation=2), dict(x=P + 8), UNSUPPORTED),
    ("fwd", dict(y_step=1, y_ih=16, y_iw=16), {}, BADARG), ("fwd", dict(y_step=2, y_py=2, y_ih=16, y_iw=16), {}, BADARG),
    ("fwd", dict(y_step=2, y_px=-1, y_ih=16, y_iw=16), {}, BADARG), ("fwd", dict(y_step=2), {}, BADARG),
    ("fwd", dict(y_step=2, y_py=1, y_ih=15, y_iw=16), {}, BADARG), ("fwd", dict(y_step=2, y_px=1, y_ih=16, y_iw=15), {}, BADARG),
    ("fwd", desc(PLANES, y_step=2, y_ih=16, y_iw=16), {}, UNSUPPORTED), ("fwd", desc(PLANES, y_step=2), {}, BADARG),
    ("fwd", desc(SPLIT32, y_step=2, y_ih=16, y_iw=16), dict(y2=P), UNSUPPORTED),
    ("fwd", dict(y_step=2, y_ih=16, y_iw=16, y2_ld=64), Y2, UNSUPPORTED),
    ("fwd", dict(y_step=2, y_ih=16, y_iw=16, stride=2, oh=4, ow=4, y_py=9), {}, BADARG),
    ("fwd", dict(y_step=2, y_ih=16, y_iw=16, stride=2, oh=4, ow=4), {}, UNSUPPORTED),
    ("fwd", dict(y_step=2, y_ih=16, y_iw=16, in_dilation=2), {}, UNSUPPORTED),
    ("fwd", dict(y_step=2, y_ih=65536, y_iw=65536), {}, UNSUPPORTED),
    # the BatchNorm-sums request
    ("stats", {}, {}, BADARG, dict(mode=0)), ("stats", {}, {}, BADARG, dict(mode=3)), ("stats", FP32, {}, BADARG, dict(mode=0)),
    ("stats", {}, {}, BADARG, dict(groups=0)), ("stats", {}, {}, BADARG, dict(nseg=0)), ("stats", {}, {}, BADARG, dict(nseg=9)),
    ("stats", dict(flags=RELU), {}, BADARG, dict(nseg=9)),
    ("stats", FP32, {}, UNSUPPORTED), ("stats", PLANES, {}, UNSUPPORTED), ("stats", dict(flags=RELU), {}, UNSUPPORTED),
    ("stats", dict(flags=RELU2), {}, UNSUPPORTED), ("stats", dict(flags=SPLIT, split_col=32), {}, BADARG),
    ("stats", dict(cout=60, y_ld=64), {}, UNSUPPORTED), ("stats", dict(y_ld=68), {}, UNSUPPORTED),
    ("stats", {}, dict(y=P + 4), UNSUPPORTED), ("stats", dict(res_ld=68), dict(residual=P), UNSUPPORTED),
    ("stats", dict(res_ld=64), dict(residual=P + 2), UNSUPPORTED),
    ("stats", dict(cout=60, y_ld=64), {}, UNSUPPORTED, {}, dict(c0=-1)),       # (the layer's shape before the segments)
    ("stats", {}, {}, BADARG, {}, dict(c0=-1)), ("stats", {}, {}, BADARG, {}, dict(c0=8, c1=8)),
    ("stats", {}, {}, BADARG, {}, dict(c1=65)), ("stats", {}, {}, BADARG, dict(nseg=2)),   # (the second segment is empty)
    ("stats", {}, {}, BADARG, dict(mode=BWD), {}), ("stats", {}, {}, BADARG, dict(mode=BWD), dict(z=P, z_ld=63)),
    ("stats", {}, {}, BADARG, dict(mode=BWD), desc(BWD_SEG, scale=P)), ("stats", {}, {}, BADARG, dict(mode=BWD), desc(BWD_SEG, shift=P)),
    ("stats", {}, {}, ALIGN, dict(mode=BWD), dict(z=P, z_ld=68)), ("stats", {}, {}, ALIGN, dict(mode=BWD), dict(z=P + 2, z_ld=64)),
    ("stats", {}, {}, BADARG, dict(mode=BWD), dict(z=P + 2, z_ld=63)),
    ("stats", {}, {}, BADARG, dict(mode=BWD), desc(BWD_SEG, c1=72)),
    # the fused max pool
    ("fwd", dict(flags=RELU | POOL | POOL_SAME), {}, BADARG), ("fwd", dict(flags=RELU | POOL_ACT2), {}, BADARG),
    ("fwd", dict(flags=RELU | POOL | POOL_ACT2), {}, BADARG), ("fwd", dict(flags=RELU | POOL | POOL_ACT2), dict(scale2=P), BADARG),
    ("fwd", desc(PLANES, flags=RELU | POOL | POOL_ACT2), dict(scale2=P, shift2=P), UNSUPPORTED),
    ("fwd", desc(PLANES, flags=RELU | POOL | POOL_ACT2), {}, BADARG),
    ("fwd", desc(SPLIT32, flags=SPLIT | RELU | POOL), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(SPLIT32, flags=SPLIT | RELU | POOL | POOL_SAME), dict(y2=P), BADARG),
    ("fwd", dict(flags=RELU | POOL, y2_ld=64), Y2, UNSUPPORTED), ("fwd", dict(flags=RELU | POOL, res_ld=64), dict(residual=P), UNSUPPORTED),
    ("stats", dict(flags=POOL), {}, UNSUPPORTED), ("xpre", dict(flags=RELU | POOL), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL, y_step=2, y_ih=16, y_iw=16), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL, in_dilation=2), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL, ih=2, iw=8, oh=2), {}, UNSUPPORTED), ("fwd", dict(flags=RELU | POOL, ih=8, iw=2, ow=2), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL_SAME, ih=7, oh=7), {}, UNSUPPORTED), ("fwd", dict(flags=RELU | POOL_SAME), {}, UNSUPPORTED),
    ("fwd", flags(FP32, RELU | POOL), {}, UNSUPPORTED), ("fwd", flags(PLANES, RELU | POOL_SAME), {}, UNSUPPORTED),
    ("fwd", flags(XP3, RELU | POOL), {}, UNSUPPORTED), ("fwd", flags(PLANES, RELU | POOL | Y_P3), {}, UNSUPPORTED),
    ("fwd", desc(PLANES, flags=RELU | POOL, math_mode=_lib.GV_MATH_BF16X2), {}, UNSUPPORTED),
    # ... is served for two layer classes only (16-bit: 32 -> 64 with a plain ReLU, the 3-channel stems; fp32 planes: 32 -> 64)
    ("fwd", dict(flags=POOL), {}, UNSUPPORTED), ("fwd", dict(flags=RELU | POOL, cout=32, y_ld=32), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL, relu_cols=32), {}, UNSUPPORTED), ("fwd", dict(flags=RELU | POOL, y_ld=68), {}, UNSUPPORTED),
    ("fwd", dict(flags=RELU | POOL), dict(x=P + 8), UNSUPPORTED), ("fwd", dict(flags=RELU | POOL, tile_cfg=1), {}, UNSUPPORTED),
    ("fwd", desc(PLANES, flags=RELU | POOL, cin=64, x_ld=64), {}, UNSUPPORTED), ("fwd", desc(PLANES, flags=RELU | POOL), dict(x=P + 4), UNSUPPORTED),
    # pre-activation on load
    ("xpre", FP32, {}, UNSUPPORTED), ("xpre", PLANES, {}, UNSUPPORTED), ("xpre", XP3, {}, UNSUPPORTED), ("xpre", {}, {}, UNSUPPORTED),
    ("xpre", desc(ONE_ONE, pad_t=1), {}, UNSUPPORTED), ("xpre", desc(ONE_ONE), dict(x=P + 8), UNSUPPORTED),
    ("xpre", desc(ONE_ONE, cin=2056, x_ld=2056), {}, UNSUPPORTED), ("xpre", desc(ONE_ONE, in_dilation=2), {}, UNSUPPORTED),
] + [("xpre", desc(ONE_ONE, tile_cfg=t + 1), {}, UNSUPPORTED) for t in (2, 3, 4, 5, 9, 10, 11, 13, 37, 38, 48)] + [
    ("xpre", desc(ONE_ONE, tile_cfg=13), {}, UNSUPPORTED),           # the special index: the streaming form serves cin = 4 * cout only
    ("xpre", desc(ONE_ONE, tile_cfg=13, cin=256, x_ld=256, flags=RELU, y_ld=68), {}, UNSUPPORTED),
    ("xpre", desc(ONE_ONE, tile_cfg=50), {}, BADARG),
    # 32-bit element offsets of the vector loaders
    ("fwd", dict(nb=65536, ih=32, iw=32, oh=32, ow=32, x_ld=64), {}, UNSUPPORTED),
    ("fwd", desc(PLANES, nb=65536, ih=32, iw=32, oh=32, ow=32, x_ld=64), {}, UNSUPPORTED),
    # three-plane input: whole 16-channel groups, aligned pixels, the staged epilogue's destinations
    ("fwd", desc(XP3, cin=40, x_ld=48), {}, UNSUPPORTED), ("fwd", desc(XP3, x_ld=40), {}, UNSUPPORTED), ("fwd", XP3, dict(x=P + 8), UNSUPPORTED),
    ("fwd", desc(XP3, y2_ld=64), Y2, UNSUPPORTED), ("fwd", desc(XP3, SPLIT32, flags=X_P3 | SPLIT, split_col=28, y_ld=28, y2_ld=36), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(XP3, SPLIT32, flags=X_P3 | SPLIT, y_ld=34), dict(y2=P), UNSUPPORTED),
    ("fwd", desc(XP3, SPLIT32, flags=X_P3 | SPLIT), dict(y2=P + 4), UNSUPPORTED),
    ("fwd", desc(XP3, SPLIT32, flags=X_P3 | SPLIT, cout=60, y2_ld=28), dict(y2=P), UNSUPPORTED),
]


def run(lib, entry, d, a, stats=None, seg=None):
    fn, names = ENTRY[entry]
    args = dict(ARGS)
    args.update(a)
    dp = None
    if d is not None:
        cd = _lib.ConvDesc(*dict(DESC, **d).values())
        dp = C.byref(cd)
    if entry == "stats":
        st = None
        if stats is not None:
            st = _lib.BnStats()
            for k, v in dict(STATS, **stats).items():
                setattr(st, k, v)
            for k, v in dict(SEG, **(seg or {})).items():
                setattr(st.seg[0], k, v)
        args["stats"] = C.byref(st) if st is not None else None
    return getattr(lib, fn)(dp, *[args[n] for n in names], None)


def test_conv_entry_argument_codes():
    lib = _lib.load()
    wrong = []
    for c in CASES:
        entry, d, a, code = c[:4]
        stats = c[4] if len(c) > 4 else ({} if entry == "stats" else None)
        rc = run(lib, entry, d, a, stats, c[5] if len(c) > 5 else None)
        if rc != code:
            wrong.append((rc, c))
    assert not wrong, wrong
