"""Operands of the kernel sweeps (helper, not collected): a tensor that is a slice of a wider flat buffer, and the
comparison that prints its measured figure before it asserts."""
import torch

DEV = "cuda:0"
NAN, SENTINEL = float("nan"), -7.0


class _Slab:
    """An [npix, c] operand of pixel stride ld that starts `off` elements into a flat buffer filled with `fill` (NaN for an
    input: the neighbours must not leak in; a sentinel for an output: they must stay as they are).  `tail` more elements of
    `fill` follow the last row."""

    def __init__(self, npix, c, ld, off, tdt, fill, values=None, tail=0):
        self.buf = torch.full((npix * ld + off + tail,), fill, dtype=tdt, device=DEV)
        self.v = self.buf.as_strided((npix, c), (ld, 1), off)
        self.fill = fill
        if values is not None:
            self.v.copy_(values.reshape(npix, c))
        self.ptr = self.v.data_ptr()

    def outside_intact(self):
        if self.v.numel() == self.buf.numel():
            return True
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        m.as_strided(self.v.shape, self.v.stride(), self.v.storage_offset()).fill_(False)
        out = self.buf[m]
        return bool(torch.isnan(out).all()) if self.fill != self.fill else bool((out == self.fill).all())


def _hold(tag, what, got, want, tol, floor=0.0):
    """max |got - want| <= tol * max |want| + floor, in float64 on the device; the figure is printed first."""
    got, want = got.double(), want.double()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.reshape(want.shape) - want).abs().max())
    print("%s %-12s rel %.3e (bound %.1e)" % (tag, what, err / scale, tol))
    assert err <= tol * scale + floor, "%s %s: max|diff| %.3e vs scale %.3e (%.2e rel)" % (tag, what, err, scale, err / scale)
