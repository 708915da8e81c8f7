"""Argument codes of the filter-gradient entry points (csrc/train.hip): gv_conv2d_wgrad, gv_conv2d_wgrad_ws and the size of
their tile_cfg table.  Every call in the table is rejected before any HIP call, so this runs without a device; the codes are
literals.  Where two conditions fail in one call, the code says which check comes first."""
import ctypes as C

import torch                                       # noqa: F401  (before the library, as in the GPU test files)

from gvcnn_tf_amd import _lib

P = 4096                                           # a 16-byte aligned stand-in address: never dereferenced
F32, BF16, F16 = _lib.GV_F32, _lib.GV_BF16, _lib.GV_F16
BADARG, UNSUPPORTED = -1, -2
NUM_CFGS = 96                                      # 27 tiles + 3 strips + 61 LDS-DMA + 5 deep strips

# a 3x3 SAME 32 -> 64 layer on an 8x8 map, 16-bit storage, channels in whole 16-byte groups (the 16-bit MFMA kernels take
# it: tile_cfg is looked at); every row below changes it until a check rejects it
DESC = dict(nb=2, ih=8, iw=8, cin=32, x_ld=32, kh=3, kw=3, stride=1, pad_t=1, pad_l=1, oh=8, ow=8, cout=64, y_ld=64, res_ld=0,
            y2_ld=0, flags=0, dtype=BF16, split_col=0, tile_cfg=0, math_mode=0, in_dilation=0, relu_cols=0, y_step=0, y_py=0,
            y_px=0, y_ih=0, y_iw=0)
ARGS = dict(x=P, dz=P, dz_ld=64, dw=P, ws=P, ws_bytes=1 << 20)

# (descriptor fields that differ (None: no descriptor), arguments that differ, code): both entry points
CASES = [
    (None, {}, BADARG),
] + [({}, {n: None}, BADARG) for n in ("x", "dz", "dw")] + [({n: 0}, {}, BADARG) for n in ("nb", "cin", "cout")] + [
    ({}, dict(dz_ld=63), BADARG), (dict(x_ld=31), {}, BADARG),
    (dict(nb=0, dtype=7), {}, BADARG),                               # (sizes before the storage type)
    (dict(dtype=7), {}, UNSUPPORTED),
    # tile_cfg: 0 = the heuristic, 1 ... table size = a configuration
    (dict(tile_cfg=NUM_CFGS + 1), {}, BADARG), (dict(dtype=F16, tile_cfg=NUM_CFGS + 1), {}, BADARG),
]
# the workspace of the deterministic form is checked before everything else
WS_CASES = [(d, dict(a, **w), BADARG) for w in (dict(ws=None), dict(ws=P + 4), dict(ws_bytes=-1))
            for d, a in (({}, {}), (None, {}), (dict(dtype=7), {}), ({}, dict(x=None)))]


def run(lib, ws, d, a):
    args = dict(ARGS, **a)
    dp = None
    if d is not None:
        cd = _lib.ConvDesc(*dict(DESC, **d).values())
        dp = C.byref(cd)
    if ws:
        return lib.gv_conv2d_wgrad_ws(dp, args["x"], args["dz"], args["dz_ld"], args["dw"], args["ws"], args["ws_bytes"], None)
    return lib.gv_conv2d_wgrad(dp, args["x"], args["dz"], args["dz_ld"], args["dw"], None)


def test_wgrad_entry_argument_codes():
    lib = _lib.load()
    wrong = []
    for ws, cases in ((False, CASES), (True, CASES + WS_CASES)):
        for d, a, code in cases:
            rc = run(lib, ws, d, a)
            if rc != code:
                wrong.append((rc, ws, d, a))
    assert not wrong, wrong


def test_wgrad_table_size():
    lib = _lib.load()
    assert [lib.gv_conv2d_wgrad_num_cfgs(dt) for dt in (BF16, F16, F32)] == [NUM_CFGS, NUM_CFGS, 0]
