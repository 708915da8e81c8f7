"""tests/pool_train_ref.py (the ordered reference the training-pool kernels are held to, tests/test_gpu_pool_train.py)
against statements written from the definition: the recorded byte is the row-major index of the first maximum among a
window's taps inside the image, and the backward is torch autograd's wherever no window ties.  Gradients are multiples of
1/4 below 8 in magnitude, so every sum of up to nine of them is exact in any order and the comparison is np.array_equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_train_ref as TR                     # (tests/pool_train_ref.py)

# kh, kw, stride, (pad_t, pad_l), (ih, iw), (oh, ow): the geometries of the kernel sweep
GEOMS = [(3, 3, 2, (0, 0), (7, 9), (3, 4)), (3, 3, 2, (0, 0), (8, 6), (3, 2)), (3, 3, 2, (0, 0), (12, 10), (6, 5)),
         (3, 3, 2, (1, 1), (11, 9), (6, 5)), (3, 3, 1, (1, 1), (5, 4), (5, 4)), (1, 1, 2, (0, 0), (9, 8), (5, 4)),
         (2, 2, 2, (0, 0), (5, 7), (2, 3)), (1, 3, 1, (0, 1), (4, 6), (4, 6)), (3, 2, 2, (0, 0), (7, 6), (3, 3))]


def _x(hw, c, ties):
    x = torch.randn(2, hw[0], hw[1], c, generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1])).numpy()
    if ties:
        x[0, 1:4, 1:4, :] = 0.5
        x[1, :, :, 0] = -3.0
    return x


@pytest.mark.parametrize("kh,kw,stride,pads,hw,out", GEOMS)
def test_bytes_are_the_first_maximum(kh, kw, stride, pads, hw, out):
    x = _x(hw, 3, ties=True)
    y, arg = TR.max_fwd(x, kh, kw, stride, pads, out)
    for n in range(2):
        for oy in range(out[0]):
            for ox in range(out[1]):
                for ch in range(3):
                    taps = []                                        # (row-major index, value) of the taps inside the image
                    for r in range(kh):
                        for s in range(kw):
                            iy, ix = oy * stride - pads[0] + r, ox * stride - pads[1] + s
                            if 0 <= iy < hw[0] and 0 <= ix < hw[1]:
                                taps.append((r * kw + s, x[n, iy, ix, ch]))
                    top = max(v for _, v in taps)
                    assert arg[n, oy, ox, ch] == next(i for i, v in taps if v == top)
                    assert y[n, oy, ox, ch] == top


@pytest.mark.parametrize("kh,kw,stride,pads,hw,out", GEOMS)
def test_backward_is_autograd_without_ties(kh, kw, stride, pads, hw, out):
    x = _x(hw, 3, ties=False)
    g = torch.Generator().manual_seed(7)
    dy = torch.randint(-31, 32, (2,) + out + (3,), generator=g).float() / 4
    prev = torch.randint(-31, 32, x.shape, generator=g).float() / 4
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    # -inf up to the last window's end on every side that has padding; a VALID window never reaches past the image
    bottom = max((out[0] - 1) * stride - pads[0] + kh - hw[0], 0)
    right = max((out[1] - 1) * stride - pads[1] + kw - hw[1], 0)
    y = F.max_pool2d(F.pad(xt, (pads[1], right, pads[0], bottom), value=float("-inf")), (kh, kw), stride)
    assert tuple(y.shape[2:]) == out
    y.backward(dy.permute(0, 3, 1, 2))
    want = xt.grad.permute(0, 2, 3, 1).numpy()
    _, arg = TR.max_fwd(x, kh, kw, stride, pads, out)
    fold, covered = TR.max_bwd(arg, dy.numpy(), hw, kh, kw, stride, pads)
    assert np.array_equal(TR.finish(fold, covered), want)
    assert np.array_equal(TR.finish(fold, covered, prev.numpy()), prev.numpy() + want)
    # what no window covers: exactly the pixels autograd never reaches, for any dy
    reach = np.zeros(hw, bool)
    for oy in range(out[0]):
        for ox in range(out[1]):
            reach[max(oy * stride - pads[0], 0):oy * stride - pads[0] + kh, max(ox * stride - pads[1], 0):ox * stride - pads[1] + kw] = True
    assert np.array_equal(covered, reach)


@pytest.mark.parametrize("kh,kw,stride,pads,hw,out", GEOMS)
def test_average_restatement_is_autograd(kh, kw, stride, pads, hw, out):
    """avg_bwd64 against autograd through the definition, sum of the taps inside the image / their number, in float64."""
    dy = torch.randn(2, *out, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    xt = torch.zeros(2, hw[0], hw[1], 3, dtype=torch.float64, requires_grad=True)
    y = torch.stack([torch.stack([sum(xt[:, iy, ix] for _, _, iy, ix in taps) / len(taps)
                                  for oy, ox, taps in TR.windows(hw[0], hw[1], kh, kw, stride, pads, out) if oy == row], 1)
                     for row in range(out[0])], 1)
    y.backward(dy)
    val, mag, terms, covered = TR.avg_bwd64(dy.numpy(), hw, kh, kw, stride, pads)
    assert np.allclose(val, xt.grad.numpy(), rtol=0, atol=1e-14)
    assert (mag >= np.abs(val) - 1e-14).all() and np.array_equal(covered, terms > 0)
