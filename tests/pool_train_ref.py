"""Ordered fp32 reference of the training pools (helper, not collected): csrc/pool_train.hip restated in numpy float32 in the
kernels' own order, so that a device result can be compared with np.array_equal.

    forward      y = the window's maximum; the recorded byte is the row-major tap r * kw + s of its FIRST maximum
    backward     per input pixel a left fold from +0.f over the windows that elected it, oy ascending then ox ascending
                 (a window that did not elect the pixel adds 0.f, which changes no bit: no partial sum is -0.f)
    store form   dx = the fold; a pixel no window covers is 0
    accumulate   dx = previous dx (widened) + the fold; a pixel no window covers keeps its dx
    16-bit       one round-to-nearest-even into the storage type at the end (the caller rounds: torch's .to(dtype))

The recomputing backward (gv_pool2d_bwd) and the one that reads the recorded bytes (gv_pool2d_bwd_argmax) elect the same
pixel, so one statement serves both.  The average backward folds g * (1.f / cnt), which the device contracts to an FMA:
numpy cannot state that, so avg_bwd64 gives the float64 value and the magnitudes a bound is computed from.
Every input is finite here (NaN only around the slices).
"""
import numpy as np

F32 = np.float32


def windows(ih, iw, kh, kw, stride, pads, out_hw):
    """(oy, ox, [(r, s, iy, ix) of the taps inside the image]) of every window, oy ascending then ox ascending."""
    for oy in range(out_hw[0]):
        for ox in range(out_hw[1]):
            taps = [(r, s, oy * stride - pads[0] + r, ox * stride - pads[1] + s) for r in range(kh) for s in range(kw)]
            yield oy, ox, [t for t in taps if 0 <= t[2] < ih and 0 <= t[3] < iw]


def max_fwd(x, kh, kw, stride, pads, out_hw):
    """x [nb, ih, iw, c] float32 -> (y [nb, oh, ow, c] float32, bytes [nb, oh, ow, c] uint8)."""
    x = np.asarray(x, dtype=F32)
    nb, ih, iw, c = x.shape
    y = np.empty((nb,) + tuple(out_hw) + (c,), F32)
    arg = np.empty(y.shape, np.uint8)
    for oy, ox, taps in windows(ih, iw, kh, kw, stride, pads, out_hw):
        best = np.full((nb, c), -np.inf, F32)
        a = np.full((nb, c), -1, np.int32)
        for r, s, iy, ix in taps:
            v = x[:, iy, ix]
            take = (v > best) | (a < 0)
            best = np.where(take, v, best)
            a = np.where(take, r * kw + s, a)
        y[:, oy, ox], arg[:, oy, ox] = best, a
    return y, arg


def max_bwd(arg, dy, in_hw, kh, kw, stride, pads):
    """bytes and dy [nb, oh, ow, c] -> (the fold [nb, ih, iw, c] float32, covered [ih, iw] bool)."""
    dy = np.asarray(dy, dtype=F32)
    nb, oh, ow, c = dy.shape
    ih, iw = in_hw
    fold = np.zeros((nb, ih, iw, c), F32)
    covered = np.zeros((ih, iw), bool)
    for oy, ox, taps in windows(ih, iw, kh, kw, stride, pads, (oh, ow)):
        for r, s, iy, ix in taps:
            fold[:, iy, ix] = fold[:, iy, ix] + np.where(arg[:, oy, ox] == r * kw + s, dy[:, oy, ox], F32(0))
            covered[iy, ix] = True
    assert fold.dtype == F32
    return fold, covered


def finish(fold, covered, prev=None):
    """The tail in float32, before the one rounding into the storage type.  prev: the accumulate form's dx (float32)."""
    m = covered[None, :, :, None]
    if prev is None:
        return np.where(m, F32(0) + fold, F32(0))
    prev = np.asarray(prev, dtype=F32)
    return np.where(m, prev + fold, prev)


def avg_bwd64(dy, in_hw, kh, kw, stride, pads, prev=None):
    """dy [nb, oh, ow, c] -> float64 (value, sum of the magnitudes of its terms) [nb, ih, iw, c] and (number of terms,
    covered) [ih, iw].  A term is dy / #valid taps of a covering window, and in the accumulate form the previous dx."""
    dy = np.asarray(dy, dtype=np.float64)
    nb, oh, ow, c = dy.shape
    ih, iw = in_hw
    val = np.zeros((nb, ih, iw, c))
    mag = np.zeros_like(val)
    terms = np.zeros((ih, iw), np.int64)
    for oy, ox, taps in windows(ih, iw, kh, kw, stride, pads, (oh, ow)):
        for _, _, iy, ix in taps:
            val[:, iy, ix] += dy[:, oy, ox] / len(taps)
            mag[:, iy, ix] += np.abs(dy[:, oy, ox]) / len(taps)
            terms[iy, ix] += 1
    covered = terms > 0
    if prev is not None:
        prev = np.asarray(prev, dtype=np.float64)
        val, mag = val + prev, mag + np.where(covered[None, :, :, None], np.abs(prev), 0.0)
        terms = terms + covered
    return val, mag, terms, covered
