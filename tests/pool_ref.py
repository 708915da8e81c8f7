"""Ordered fp32 reference of the forward pools (helper, not collected): csrc/pool.hip restated in numpy float32 with the
additions in the kernels' own order, so that a device result can be compared with np.array_equal.

    max              exact whatever the order (fmaxf: a NaN tap is skipped, as np.fmax skips it)
    generic average  the valid taps folded left from 0.f, r ascending then s ascending; one division by the float count of
                     valid taps (the divisor of TF's SAME average)
    rows average     (the 3x3 / stride 1 / SAME forms, one or two output rows per thread) per input column a left fold
                     over the valid rows, ascending, from 0.f; out = (col[ox-1] + col[ox]) + col[ox+1] with a column outside
                     the image 0.f; one division by rows * cols
    ReLU             after the division
    16-bit storage   one round-to-nearest-even into the storage type at the end (the caller rounds: torch's .to(dtype))

The two-row form replaces the division by a reciprocal and one exact-remainder correction that is documented as giving
the division's bits; numpy's / is its statement here.  numpy's float32 + and / are single IEEE operations, and adding the
0.f of a tap outside the image changes no bit (no partial sum is -0.f: the folds start at +0.f), so the masked whole-array
sums below are the per-output folds element for element.
"""
import numpy as np

F32 = np.float32
MAX, AVG, AVG_RELU = 0, 1, 2                       # GV_POOL_MAX / _AVG / _AVG_RELU


def _taps(x, k, stride, pad, out, axis):
    """For tap t of k along `axis`: (x gathered at the clipped input index of every output, the mask of outputs whose tap is
    inside the image, shaped to broadcast)."""
    n = x.shape[axis]
    o = np.arange(out) * stride - pad
    shape = [1] * x.ndim
    shape[axis] = out
    for t in range(k):
        i = o + t
        yield np.take(x, np.clip(i, 0, n - 1), axis=axis), ((i >= 0) & (i < n)).reshape(shape)


def pool_generic(x, k, stride, pads, out_hw, mode):
    """x [nb, ih, iw, c] float32 -> [nb, oh, ow, c] float32: pool2d's order (every window holds a valid tap)."""
    x = np.asarray(x, dtype=F32)
    oh, ow = out_hw
    acc = np.full((x.shape[0], oh, ow, x.shape[3]), -np.inf if mode == MAX else 0.0, F32)
    cnt = np.zeros((1, oh, ow, 1), F32)
    with np.errstate(invalid="ignore"):
        for rows, rmask in _taps(x, k, stride, pads[0], oh, 1):
            for v, smask in _taps(rows, k, stride, pads[1], ow, 2):
                m = rmask & smask
                acc = np.where(m, np.fmax(acc, v), acc) if mode == MAX else acc + np.where(m, v, F32(0))
                cnt = cnt + m.astype(F32)
        if mode != MAX:
            acc = acc / cnt
            if mode == AVG_RELU:
                acc = np.fmax(acc, F32(0))
    assert acc.dtype == F32
    return acc


def avg_rows(x, relu):
    """x [nb, ih, iw, c] float32 -> the 3x3 / stride 1 / SAME average in the order of avgpool3x3s1_rows (both ROWS)."""
    x = np.asarray(x, dtype=F32)
    nb, ih, iw, c = x.shape
    with np.errstate(invalid="ignore"):
        col = np.zeros_like(x)
        for v, m in _taps(x, 3, 1, 1, ih, 1):
            col = col + np.where(m, v, F32(0))
        z = np.zeros((nb, ih, 1, c), F32)
        cp = np.concatenate([z, col, z], axis=2)
        s = (cp[:, :, 0:iw] + cp[:, :, 1:iw + 1]) + cp[:, :, 2:iw + 2]
        rows = np.minimum(np.arange(ih) + 1, ih - 1) - np.maximum(np.arange(ih) - 1, 0) + 1
        cols = np.minimum(np.arange(iw) + 1, iw - 1) - np.maximum(np.arange(iw) - 1, 0) + 1
        y = s / (rows[:, None] * cols[None, :]).astype(F32)[None, :, :, None]
        if relu:
            y = np.fmax(y, F32(0))
    assert y.dtype == F32
    return y
