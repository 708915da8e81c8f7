"""The forward pools (gv_pool2d_fwd, csrc/pool.hip) over their kernel forms and storages against tests/pool_ref.py, the
ordered fp32 restatement: the device result must EQUAL it (np.array_equal), rounded once to nearest even for 16-bit storage.

Storages: fp32, bf16, fp16, and fp32 values in the three-plane layout on the input, the output or both (p3in / p3out /
p3both).  Every operand is a channel slice of a wider buffer: NaN around an input (a neighbour that leaks in shows), a
sentinel around an output (it must stay).  Inputs are randn rounded to the storage type, so every sum is a normal number
and the restatement is exact.  nb = 2 throughout.

Case -> kernel form -> the condition that selects it (quad = 4 fp32 or 8 16-bit channels):
  3x3 / 1 SAME average, 16-bit, c % 8 == 0                     avgpool3x3s1_rows<.., 2>   two rows per thread, reciprocal form
  the same, three-plane input, c % 8 == 0                       avgpool3x3s1_rows<P3Px<8>, .., 2>
  the same, three-plane input c = 20; fp32 input (plain, p3out)  avgpool3x3s1_rows<.., 1>   one row per thread, division
  3x3 / 2 VALID max, plain storage, gv_pool2d_set_rows(1)       maxpool3x3s2_rows<.., 4>   (0: pool2d)
  every other geometry, and every pool whose c, strides or bases break the 16-byte walk      pool2d (vector or scalar)
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gvcnn_tf_amd import _lib, p3              # noqa: E402
from oracle import backbone as OB               # noqa: E402
import pool_ref as PR                           # noqa: E402   (tests/pool_ref.py)
from slab import DEV, NAN, SENTINEL             # noqa: E402   (tests/slab.py)

MAX, AVG, AVG_RELU = _lib.GV_POOL_MAX, _lib.GV_POOL_AVG, _lib.GV_POOL_AVG_RELU
assert (MAX, AVG, AVG_RELU) == (PR.MAX, PR.AVG, PR.AVG_RELU)
# name: (dtype code, torch dtype, three-plane input, three-plane output)
STORAGES = {"f32": (_lib.GV_F32, torch.float32, False, False), "bf16": (_lib.GV_BF16, torch.bfloat16, False, False),
            "f16": (_lib.GV_F16, torch.float16, False, False), "p3in": (_lib.GV_F32, torch.float32, True, False),
            "p3out": (_lib.GV_F32, torch.float32, False, True), "p3both": (_lib.GV_F32, torch.float32, True, True)}
PLAIN = ["f32", "bf16", "f16"]


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def quad(storage):
    return 16 // torch.empty(0, dtype=STORAGES[storage][1]).element_size()


def values(storage, shape, *key):
    """randn rounded to the storage type, as float32 on the host; seeded by the case."""
    g = torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(shape + key)) % (2 ** 31))
    return torch.randn(*shape, generator=g).to(STORAGES[storage][1]).float()


def _wide(vals, shape, ld, off, tdt, planes, fill):
    """A [nb, h, w, ld] buffer of `fill` with vals (or nothing) in channels [off, off + c); (buffer, pointer to the slice)."""
    wide = torch.full(shape[:3] + (ld,), fill, dtype=torch.float32, device=DEV)
    if vals is not None:
        wide[..., off:off + shape[3]] = vals.to(DEV)
    buf = p3.to_p3(wide) if planes else wide.to(tdt)
    return buf, buf.data_ptr() + off * (6 if planes else buf.element_size())


def slices(storage, c, kind="vec"):
    """(x_ld, x_off, y_ld, y_off) of the channel slices.  vec: every stride and offset keeps the 16-byte walk (whole
    16-channel groups on a three-plane side); ld1: a pixel stride one element over c; off1: a base one element in."""
    _, _, xp3, yp3 = STORAGES[storage]
    q = quad(storage)

    def one(planes, pad):
        if planes:
            return -(-c // 16) * 16 + 16 * pad, 16
        return {"vec": (c + pad * q, q), "ld1": (c + 1, 0), "off1": (c + pad * q, 1)}[kind]
    return one(xp3, 2) + one(yp3, 1)


def vec_ok(storage, c, sl):
    """The 16-byte walk is possible (a three-plane operand allows nothing else)."""
    _, _, xp3, yp3 = STORAGES[storage]
    q = quad(storage)
    return xp3 or yp3 or (c % q == 0 and all(v % q == 0 for v in sl))


def run_pool(storage, x, k, stride, pads, out_hw, mode, sl):
    """x [nb, ih, iw, c] float32 (host) -> the device pool's output slice as a float32 ndarray; the surroundings of both
    slices are checked here."""
    code, tdt, xp3, yp3 = STORAGES[storage]
    nb, ih, iw, c = x.shape
    x_ld, x_off, y_ld, y_off = sl
    xbuf, xptr = _wide(x, tuple(x.shape), x_ld, x_off, tdt, xp3, NAN)
    ybuf, yptr = _wide(None, (nb,) + tuple(out_hw) + (c,), y_ld, y_off, tdt, yp3, SENTINEL)
    d = _lib.PoolDesc(nb, ih, iw, c, x_ld, k, k, stride, pads[0], pads[1], out_hw[0], out_hw[1], y_ld,
                      mode | (_lib.GV_POOL_X_P3 if xp3 else 0) | (_lib.GV_POOL_Y_P3 if yp3 else 0), code)
    _lib.check(lib().gv_pool2d_fwd(C.byref(d), xptr, yptr, st()), "gv_pool2d_fwd")
    torch.cuda.synchronize()
    y = p3.from_p3(ybuf) if yp3 else ybuf.float()
    assert bool((y[..., :y_off] == SENTINEL).all()) and bool((y[..., y_off + c:] == SENTINEL).all()), "output surroundings"
    return y[..., y_off:y_off + c].cpu().numpy()


def expect(storage, x, k, stride, pads, out_hw, mode, rows_form):
    """The ordered restatement on the stored values, rounded once into a 16-bit storage type."""
    xn = x.numpy()
    ref = PR.avg_rows(xn, mode == AVG_RELU) if rows_form else PR.pool_generic(xn, k, stride, pads, out_hw, mode)
    return torch.from_numpy(ref).to(STORAGES[storage][1]).float().numpy()


def check(tag, storage, x, k, stride, pads, out_hw, mode, sl):
    c = x.shape[3]
    avg3 = mode != MAX and (k, stride, tuple(pads), tuple(out_hw)) == (3, 1, (1, 1), tuple(x.shape[1:3]))
    got = run_pool(storage, x, k, stride, pads, out_hw, mode, sl)
    want = expect(storage, x, k, stride, pads, out_hw, mode, avg3 and vec_ok(storage, c, sl))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN in other places than the restatement's" % tag
    assert np.array_equal(np.where(nan, 0, got), np.where(nan, 0, want)), "%s: %d of %d values differ" % (
        tag, int((np.where(nan, 0, got) != np.where(nan, 0, want)).sum()), got.size)
    return got


# ---- the case lists (tools compare two builds of the library on the same cases) -----------------------------------------
def average_rows_cases(storage):
    """ih in {1, 2, 3} (a pair's second row missing, one pair, a pair and a half) x iw in {1, 4, 5, 6} (one ragged group
    of four, one whole group, a group and one / two columns) x AVG / AVG_RELU, at the channel counts of the storage."""
    cs = {"f32": (4, 12), "bf16": (8, 16), "f16": (8, 16)}.get(storage, (16, 32, 20))
    for ih in (1, 2, 3):
        for iw in (1, 4, 5, 6):
            for c in cs:
                for mode in (AVG, AVG_RELU):
                    yield ("avg rows %s %dx%dx%d mode %d" % (storage, ih, iw, c, mode), values(storage, (2, ih, iw, c), mode), 3, 1,
                           (1, 1), (ih, iw), mode, slices(storage, c))


def max_rows_cases(storage):
    """oh in {1, 4, 5} (a ragged only block of RH = 4, one whole block, a block and one row; ih = 9 and 10 both give 4),
    odd and even iw, three quads of channels."""
    for ih in (3, 9, 10, 11):
        for iw in (7, 8):
            c = 3 * quad(storage)
            yield ("max rows %s %dx%d" % (storage, ih, iw), values(storage, (2, ih, iw, c)), 3, 2, (0, 0),
                   ((ih - 3) // 2 + 1, (iw - 3) // 2 + 1), MAX, slices(storage, c))


def generic_cases(storage):
    """3x3 / 2 SAME with TF's pads ((0, 1) on even sizes, (1, 1) on odd ones), the 1x1 / 2 subsample, a 2x2 / 2 average, and
    the 3x3 / 1 SAME average where the 16-byte walk is not possible; on plain storage also c = 6 and a stride and a base
    that break the alignment."""
    geos = []
    for ih, iw in ((6, 8), (7, 5)):
        pads = (OB.same_pads(ih, 3, 2)[0], OB.same_pads(iw, 3, 2)[0])
        geos += [(ih, iw, 3, 2, pads, (-(-ih // 2), -(-iw // 2)), m) for m in (MAX, AVG, AVG_RELU)]
    geos += [(7, 6, 1, 2, (0, 0), (4, 3), MAX), (6, 7, 2, 2, (0, 0), (3, 3), AVG), (3, 5, 3, 1, (1, 1), (3, 5), AVG)]
    q = quad(storage)
    forms = [(2 * q, "vec"), (6, "vec"), (2 * q, "ld1"), (2 * q, "off1")] if storage in PLAIN else [(20, "vec")]
    for ih, iw, k, s, pads, out_hw, mode in geos:
        for c, kind in forms:
            yield ("generic %s %dx%d k%d s%d mode %d c%d %s" % (storage, ih, iw, k, s, mode, c, kind),
                   values(storage, (2, ih, iw, c), k, s, mode), k, s, pads, out_hw, mode, slices(storage, c, kind))


def non_finite_cases(storage):
    """The windows of an activation that overflowed: one with +inf averages to +inf, one with -inf to -inf, one with a
    NaN to NaN — what the division gives; the reciprocal form of the two-row kernel must not turn an infinity into a NaN.
    Two quads of channels (the rows forms) and c = 6 (pool2d)."""
    for c in (2 * quad(storage), 6):
        x = values(storage, (2, 15, 14, c))
        x[0, 4, 4, 0] = float("inf")
        x[0, 10, 9, 1] = float("-inf")
        x[1, 7, 7, 2] = float("nan")
        yield ("non-finite %s c%d" % (storage, c), x, 3, 1, (1, 1), (15, 14), AVG, slices(storage, c))


# ---- the tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", list(STORAGES))
def test_average_rows_forms_bit_for_bit(storage):
    """The 3x3 / stride 1 / SAME average at average_rows_cases: per column the valid rows ascending, (col + col) + col, one
    division by rows * cols, ReLU after it — the same bits from the one-row form (division) and the two-row form
    (reciprocal and correction), from every storage and every pairing of three-plane and fp32 sides."""
    for case in average_rows_cases(storage):
        check(case[0], storage, *case[1:])


@pytest.mark.parametrize("storage", PLAIN)
def test_max_rows_form_equals_the_one_output_form(storage):
    """The 3x3 / stride 2 / VALID max pool at max_rows_cases with gv_pool2d_set_rows 1 (four outputs per thread) and 0 (one):
    both equal the restatement, hence each other."""
    for case in max_rows_cases(storage):
        outs = []
        for rows in (1, 0):
            lib().gv_pool2d_set_rows(rows)
            try:
                outs.append(check("%s rows %d" % (case[0], rows), storage, *case[1:]))
            finally:
                lib().gv_pool2d_set_rows(1)
        assert np.array_equal(outs[0], outs[1]), case[0]


@pytest.mark.parametrize("storage", list(STORAGES))
def test_generic_pool_vector_and_scalar_forms_bit_for_bit(storage):
    """pool2d at generic_cases: the valid taps folded from 0.f, r then s ascending, one division by their count."""
    for case in generic_cases(storage):
        check(case[0], storage, *case[1:])


def test_grid_stride_loop_of_the_scalar_walk():
    """2 x 64 x 64 x 129 fp32 outputs, one thread each on the scalar walk (c is odd): 1 056 768 threads, just over the
    4096 workgroups of 256 that a grid-stride launch is capped at, so the stride loop runs a second trip."""
    c = 129
    assert 2 * 64 * 64 * c > 4096 * 256
    check("grid stride", "f32", values("f32", (2, 64, 64, c)), 3, 1, (1, 1), (64, 64), AVG, (c + 2, 1, c + 3, 2))


@pytest.mark.parametrize("storage", PLAIN)
def test_average_of_non_finite_windows(storage):
    """non_finite_cases: NaN exactly where the restatement has it, the same values (infinities among them) elsewhere."""
    for case in non_finite_cases(storage):
        got = check(case[0], storage, *case[1:])
        assert np.isposinf(got[0, 3:6, 3:6, 0]).all() and np.isneginf(got[0, 9:12, 8:11, 1]).all() and np.isnan(got[1, 6:9, 6:9, 2]).all()
