"""tests/pool_ref.py (the ordered fp32 restatement that the device pools must equal) against oracle/backbone.py: max pools
and the subsample exactly; averages, against the oracle evaluated in float64, within one fp32 rounding per addition and
one for the division: (taps + 1) 2^-24 of the window's mean |x|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import backbone as OB
import pool_ref as PR                           # tests/pool_ref.py

U = 2.0 ** -24


def _x(nb, ih, iw, c):
    return torch.randn(nb, ih, iw, c, generator=torch.Generator().manual_seed(ih * 100 + iw * 10 + c))


@pytest.mark.parametrize("ih,iw", [(3, 3), (6, 8), (7, 5), (15, 14)])
def test_max_pools_and_subsample_equal_the_oracle(ih, iw):
    x = _x(2, ih, iw, 6)
    y = PR.pool_generic(x.numpy(), 3, 2, (0, 0), ((ih - 3) // 2 + 1, (iw - 3) // 2 + 1), PR.MAX)
    assert np.array_equal(y, OB.max_pool2d(x, 3, 2, "VALID").numpy())
    ref = OB.max_pool2d(x, 3, 2, "SAME")
    y = PR.pool_generic(x.numpy(), 3, 2, (OB.same_pads(ih, 3, 2)[0], OB.same_pads(iw, 3, 2)[0]), ref.shape[1:3], PR.MAX)
    assert np.array_equal(y, ref.numpy())
    y = PR.pool_generic(x.numpy(), 1, 2, (0, 0), (-(-ih // 2), -(-iw // 2)), PR.MAX)
    assert np.array_equal(y, x[:, ::2, ::2].numpy())


def _within(got, want64, mean_abs64, taps):
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= (taps + 1) * U * mean_abs64).all(), float((err / np.maximum(mean_abs64, 1e-300)).max() / U)


@pytest.mark.parametrize("ih,iw", [(1, 1), (1, 4), (2, 5), (3, 6), (15, 14)])
@pytest.mark.parametrize("relu", [False, True])
def test_same3_averages_in_both_orders_follow_the_oracle(ih, iw, relu):
    """The rows order and the generic order of the 3x3 / stride 1 / SAME average: the oracle's valid-tap divisor."""
    x = _x(2, ih, iw, 5)
    want = OB.avg_pool2d_same3(x.double())
    mabs = OB.avg_pool2d_same3(x.double().abs()).numpy()
    want = (torch.relu(want) if relu else want).numpy()
    _within(PR.avg_rows(x.numpy(), relu), want, mabs, 9)
    _within(PR.pool_generic(x.numpy(), 3, 1, (1, 1), (ih, iw), PR.AVG_RELU if relu else PR.AVG), want, mabs, 9)


def test_generic_average_counts_the_valid_taps_only():
    """2x2 / 2 VALID (every tap valid) and 3x3 / 2 SAME with TF's (0, 1) pads (the last row and column of windows ragged)
    against torch's average with the padding left out of the divisor."""
    x = _x(2, 6, 8, 5)
    xn = x.double().permute(0, 3, 1, 2)
    want = F.avg_pool2d(xn, 2, 2).permute(0, 2, 3, 1).numpy()
    mabs = F.avg_pool2d(xn.abs(), 2, 2).permute(0, 2, 3, 1).numpy()
    _within(PR.pool_generic(x.numpy(), 2, 2, (0, 0), (3, 4), PR.AVG), want, mabs, 4)
    assert (OB.same_pads(6, 3, 2), OB.same_pads(8, 3, 2)) == ((0, 1), (0, 1))
    pad = F.pad(xn, (0, 1, 0, 1))                                     # bottom / right only: the window grid of TF's SAME
    ones = F.pad(torch.ones_like(xn), (0, 1, 0, 1))
    cnt = F.avg_pool2d(ones, 3, 2) * 9
    want = (F.avg_pool2d(pad, 3, 2) * 9 / cnt).permute(0, 2, 3, 1).numpy()
    mabs = (F.avg_pool2d(pad.abs(), 3, 2) * 9 / cnt).permute(0, 2, 3, 1).numpy()
    _within(PR.pool_generic(x.numpy(), 3, 2, (0, 0), (3, 4), PR.AVG), want, mabs, 9)


def test_non_finite_windows_keep_what_the_division_gives():
    x = _x(1, 5, 6, 3)
    x[0, 1, 1, 0], x[0, 3, 4, 1], x[0, 2, 2, 2] = float("inf"), float("-inf"), float("nan")
    for y in (PR.avg_rows(x.numpy(), False), PR.pool_generic(x.numpy(), 3, 1, (1, 1), (5, 6), PR.AVG)):
        assert np.isposinf(y[0, 0:3, 0:3, 0]).all() and np.isneginf(y[0, 2:5, 3:6, 1]).all() and np.isnan(y[0, 1:4, 1:4, 2]).all()
        assert np.isfinite(y[0, :, :, 0]).sum() == 30 - 9
