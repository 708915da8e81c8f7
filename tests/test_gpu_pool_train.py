"""The pooling ops of the training step (gv_pool2d_fwd_argmax, gv_pool2d_bwd, gv_pool2d_bwd_argmax; csrc/pool_train.hip)
over their kernel forms and storages against tests/pool_train_ref.py, the ordered fp32 restatement.

Max pooling must EQUAL it (np.array_equal): the forward output, the recorded bytes, and the backward of both entry points
(winners recomputed from x / read from the bytes) in the store and in the accumulate form, rounded once to nearest even for
16-bit storage — every value is a single IEEE addition of storage-rounded values away from the next.  Ties are planted in
every case: a constant patch spanning several windows and one constant channel.

The average backward folds g * (1.f / cnt), contracted to an FMA on the device, which numpy cannot state.  It is held per
element to the float64 restatement within
    (terms + 2) * 2^-24 * sum |term|      one rounding per fold step, one for 1.f / cnt, one for the final addition
    + half an ulp of the storage type at the result, for 16-bit storage
where the terms are dy / cnt of the covering windows (store form: `terms` is their number) and, in the accumulate form, the
previous dx as one term more: its addition rounds like every other step of the fold.  A pixel no window covers is exact
in both forms (0, or the previous dx).

Every operand is a channel slice of a wider buffer (tests/slab.py): NaN around an input, a sentinel around an output that
must survive; the bytes sit between sentinel bytes.  nb = 2.

Geometry -> what it exercises (the block kernel owns 2x2 input pixels per thread and serves 3x3 / 2 windows):
  3x3/2 VALID (7, 9)     block kernel; the last block row has one pixel row
  3x3/2 VALID (8, 6)     the last input row and column belong to no window
  3x3/2 SAME (12, 10)    pads (0, 0) with a clipped last window: block kernel for recorded winners, gather for recomputed
  3x3/2 SAME (11, 9)     pads (1, 1): gather for both
  3x3/1 SAME (5, 4)      up to nine covering windows
  1x1/2 VALID (9, 8)     three of four pixels uncovered
  2x2/2 VALID (5, 7)     uncovered last row and column in the gather
  1x3/1 pads (0, 1)      kh != kw: the byte is r * kw + s
  3x2/2 VALID (7, 6)     the same, strided
Channel form (c, ld, slice offset, byte offset) -> walk: quads / wide: 16-byte quads; scalar: c = 5; ld12: quads on fp32,
scalar on 16-bit storage; off1: a base one element in, scalar; argoff: bytes one byte in, scalar for the ops that read or
write them.  Recomputed winners take the block kernel only with quads, recorded winners at any width.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gvcnn_tf_amd import _lib                   # noqa: E402
import pool_train_ref as TR                     # noqa: E402   (tests/pool_train_ref.py)
from slab import DEV, NAN, SENTINEL, _Slab      # noqa: E402   (tests/slab.py)

NB = 2
STORAGES = {"f32": (_lib.GV_F32, torch.float32), "bf16": (_lib.GV_BF16, torch.bfloat16), "f16": (_lib.GV_F16, torch.float16)}
# kh, kw, stride, (pad_t, pad_l), (ih, iw), (oh, ow)
GEOMS = {"3x3s2_valid_7x9": (3, 3, 2, (0, 0), (7, 9), (3, 4)), "3x3s2_valid_8x6": (3, 3, 2, (0, 0), (8, 6), (3, 2)),
         "3x3s2_same_12x10": (3, 3, 2, (0, 0), (12, 10), (6, 5)), "3x3s2_same_11x9": (3, 3, 2, (1, 1), (11, 9), (6, 5)),
         "3x3s1_same_5x4": (3, 3, 1, (1, 1), (5, 4), (5, 4)), "1x1s2_valid_9x8": (1, 1, 2, (0, 0), (9, 8), (5, 4)),
         "2x2s2_valid_5x7": (2, 2, 2, (0, 0), (5, 7), (2, 3)), "1x3s1_pad01_4x6": (1, 3, 1, (0, 1), (4, 6), (4, 6)),
         "3x2s2_valid_7x6": (3, 2, 2, (0, 0), (7, 6), (3, 3))}
# c, ld, offset of the slice in elements, offset of the bytes
FORMS = {"quads": (16, 16, 0, 0), "wide": (24, 40, 8, 0), "scalar": (5, 7, 1, 0), "ld12": (8, 12, 4, 0),
         "off1": (16, 24, 1, 0), "argoff": (16, 16, 0, 1)}
ARG_FILL = 0xEE


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def operands(geom, c, storage):
    """(x, dy, previous dx) as float32 on the host, rounded to the storage type; ties planted in x."""
    _, _, _, _, (ih, iw), (oh, ow) = GEOMS[geom]
    tdt = STORAGES[storage][1]
    g = torch.Generator().manual_seed(sorted(GEOMS).index(geom) * 1000 + c * 10 + sorted(STORAGES).index(storage))
    x = torch.randn(NB, ih, iw, c, generator=g).to(tdt).float()
    x[0, 1:4, 1:4, :] = 0.5
    x[1, :, :, 0] = -3.0
    dy = torch.randn(NB, oh, ow, c, generator=g).to(tdt).float()
    prev = torch.randn(NB, ih, iw, c, generator=g).to(tdt).float()
    return x, dy, prev


@functools.lru_cache(maxsize=None)
def max_reference(geom, c, storage):
    """(y, bytes, dx of the store form, dx of the accumulate form) of the restatement, rounded into the storage type."""
    kh, kw, stride, pads, hw, out = GEOMS[geom]
    x, dy, prev = (t.numpy() for t in operands(geom, c, storage))
    y, arg = TR.max_fwd(x, kh, kw, stride, pads, out)
    fold, covered = TR.max_bwd(arg, dy, hw, kh, kw, stride, pads)
    rnd = lambda a: torch.from_numpy(a).to(STORAGES[storage][1]).float().numpy()
    return rnd(y), arg, rnd(TR.finish(fold, covered)), rnd(TR.finish(fold, covered, prev))


@functools.lru_cache(maxsize=None)
def avg_reference(geom, c, storage, accumulate):
    kh, kw, stride, pads, hw, _ = GEOMS[geom]
    _, dy, prev = (t.numpy() for t in operands(geom, c, storage))
    return TR.avg_bwd64(dy, hw, kh, kw, stride, pads, prev if accumulate else None)


def desc(geom, form, storage, mode):
    kh, kw, stride, pads, (ih, iw), (oh, ow) = GEOMS[geom]
    c, ld, _, _ = FORMS[form]
    return _lib.PoolDesc(NB, ih, iw, c, ld, kh, kw, stride, pads[0], pads[1], oh, ow, ld, mode, STORAGES[storage][0])


def slab(form, storage, shape, fill, values=None):
    c, ld, off, _ = FORMS[form]
    return _Slab(shape[0] * shape[1] * shape[2], c, ld, off, STORAGES[storage][1], fill, values, tail=3)


def host(s, shape):
    return s.v.float().cpu().numpy().reshape(shape)


def run_backward(entry, geom, form, storage, mode, first, dy, store):
    """dx [nb, ih, iw, c] float32 of gv_pool2d_bwd (first = x) or gv_pool2d_bwd_argmax (first = the bytes); the accumulate
    form starts from the case's previous dx, the store form from NaN."""
    _, _, _, _, (ih, iw), _ = GEOMS[geom]
    c, ld, _, _ = FORMS[form]
    prev = operands(geom, c, storage)[2]
    start = torch.full_like(prev, NAN) if store else prev
    dx = slab(form, storage, (NB, ih, iw), SENTINEL, start.to(DEV))
    d = desc(geom, form, storage, mode | (_lib.GV_POOL_BWD_STORE if store else 0))
    _lib.check(getattr(lib(), entry)(C.byref(d), first, dy.ptr, ld, dx.ptr, ld, st()), entry)
    torch.cuda.synchronize()
    assert dx.outside_intact(), "%s wrote outside its dx slice" % entry
    return host(dx, (NB, ih, iw, c))


def run_max(geom, form, storage):
    """Every output of the max-pool entry points on one case: y, the bytes, and dx of (recomputed, recorded) x (store,
    accumulate)."""
    _, _, _, _, (ih, iw), (oh, ow) = GEOMS[geom]
    c, ld, _, arg_off = FORMS[form]
    xv, dyv, _ = operands(geom, c, storage)
    x = slab(form, storage, (NB, ih, iw), NAN, xv.to(DEV))
    y = slab(form, storage, (NB, oh, ow), SENTINEL)
    dy = slab(form, storage, (NB, oh, ow), NAN, dyv.to(DEV))
    n = NB * oh * ow * c
    argbuf = torch.full((n + 16,), ARG_FILL, dtype=torch.uint8, device=DEV)
    argptr = argbuf.data_ptr() + arg_off
    d = desc(geom, form, storage, _lib.GV_POOL_MAX)
    _lib.check(lib().gv_pool2d_fwd_argmax(C.byref(d), x.ptr, y.ptr, argptr, st()), "gv_pool2d_fwd_argmax")
    torch.cuda.synchronize()
    assert y.outside_intact(), "the forward wrote outside its y slice"
    assert bool((argbuf[:arg_off] == ARG_FILL).all()) and bool((argbuf[arg_off + n:] == ARG_FILL).all()), "bytes surroundings"
    out = {"y": host(y, (NB, oh, ow, c)), "arg": argbuf[arg_off:arg_off + n].cpu().numpy().reshape(NB, oh, ow, c)}
    for store in (1, 0):
        tag = "store" if store else "acc"
        out["recomputed_" + tag] = run_backward("gv_pool2d_bwd", geom, form, storage, _lib.GV_POOL_MAX, x.ptr, dy, store)
        out["recorded_" + tag] = run_backward("gv_pool2d_bwd_argmax", geom, form, storage, _lib.GV_POOL_MAX, argptr, dy, store)
    return out


def run_avg(geom, form, storage):
    _, _, _, _, _, (oh, ow) = GEOMS[geom]
    c = FORMS[form][0]
    dy = slab(form, storage, (NB, oh, ow), NAN, operands(geom, c, storage)[1].to(DEV))
    return {"avg_" + ("store" if store else "acc"): run_backward("gv_pool2d_bwd", geom, form, storage, _lib.GV_POOL_AVG, None,
                                                                 dy, store) for store in (1, 0)}


def same(tag, got, want):
    assert np.array_equal(got, want), "%s: %d of %d values differ" % (tag, int((got != want).sum()), got.size)


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_max_pool_equals_the_restatement(geom, form, storage):
    y, arg, dx_store, dx_acc = max_reference(geom, FORMS[form][0], storage)
    got = run_max(geom, form, storage)
    tag = "%s %s %s" % (geom, form, storage)
    same(tag + " y", got["y"], y)
    same(tag + " bytes", got["arg"], arg)
    for winners in ("recomputed", "recorded"):
        same("%s %s store" % (tag, winners), got[winners + "_store"], dx_store)
        same("%s %s accumulate" % (tag, winners), got[winners + "_acc"], dx_acc)


def storage_ulp(storage, v):
    """The spacing of the 16-bit storage type at |v| (its subnormal spacing below the normal range)."""
    mant, emin = {"bf16": (7, -126), "f16": (10, -14)}[storage]
    e = np.frexp(np.maximum(np.abs(v), 2.0 ** emin))[1] - 1
    return np.ldexp(1.0, e - mant)


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_avg_pool_backward_within_its_bound(geom, form, storage):
    c = FORMS[form][0]
    got = run_avg(geom, form, storage)
    prev = operands(geom, c, storage)[2].numpy()
    for accumulate in (0, 1):
        g = got["avg_acc" if accumulate else "avg_store"].astype(np.float64)
        val, mag, terms, covered = avg_reference(geom, c, storage, accumulate)
        bound = (terms[None, :, :, None] + 2) * 2.0 ** -24 * mag
        if storage != "f32":
            bound = bound + 0.5 * storage_ulp(storage, np.maximum(np.abs(g), np.abs(val)))
        err = np.abs(g - val)
        m = covered[None, :, :, None] & np.ones(g.shape, bool)
        print("%s %s %s %s: max err / bound %.3f" % (geom, form, storage, "accumulate" if accumulate else "store",
                                                      float((err[m] / bound[m]).max())))
        assert (err[m] <= bound[m]).all(), "%d of %d covered values beyond the bound" % (int((err[m] > bound[m]).sum()), int(m.sum()))
        same("uncovered pixels", g[~m], (prev.astype(np.float64) if accumulate else np.zeros(g.shape))[~m])
