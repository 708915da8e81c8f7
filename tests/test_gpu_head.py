"""The grouping head's kernels over their launch geometries (csrc/grouping.hip, one template per op for every storage type;
the element-wise ones in csrc/pool.hip, the pooling backward in csrc/train.hip) against tests/head_ref.py: an fp64
restatement of the stored values, and an ordered fp32 one where the kernel fixes the order of its operations.

Operands are slices of wider flat buffers (tests/slab.py): inputs surrounded by NaN, outputs by a sentinel.  Reductions also
run on small integers (|x| <= 4, |k| <= 3, fewer than 2^20 terms: every partial sum is an integer below 2^24, asserted on the
reference), where the result must equal the numpy fp32 formula bit for bit whatever the order of the additions.

Random values are held to  |got - want| <= (d + 2) 2^-23 sum |terms|  for a sum whose longest chain of fp32 additions is d
(read off the loop structure, computed from the geometry), plus 2^-24 of the operands of each trailing division / bias
addition, plus one rounding of the storage type for a 16-bit output (2^-8 / 2^-11 of the tensor's scale).  The scores go
through the device's logf and expf: no accuracy table of the device library is at hand, so 2 ulp each is ASSUMED; lg = ln r
then carries 2 * 2^-23 |ln r| absolute, exp(-lg) that plus 2 * 2^-23 relative, 1 + e and 1 / x half an ulp each, and
|d score / score| <= |de / e|:  (4 |ln r| + 6) 2^-24 relative.  A result below the smallest normal fp32 (a subnormal r) is
held to 2^-126 absolute: the relative bound is one of normal numbers, and expf(-ln r) overflows for r < 2^-128.

Case -> kernel form -> the condition that selects it (chunk = 4 elements of fp32, 8 of a 16-bit type; cg = cr / chunk):
  score idle / tail3 / trip / straddle / trips / hw1   vector walk of view_score_partial<E, T>      cr, raw_ld % chunk == 0
      and raw, kernel 16-byte aligned; hw * cg = 128 (idle threads), 600 (tail loop only, 3 trips), 1024 (one unrolled
      trip, no tail), 1176 (a trip, then a tail for threads < 152; hw = 49, cg = 24: a trip's 4 chunks in different
      pixels), 5000 (4 trips + tail), hw = 1;  +ld1 / +ld2: raw_ld = cr + 1 / 2 chunks;  +16B: operands 16 bytes in
  score cr30 / ld34 / base1                            scalar branch                               cr % chunk != 0 /
      raw_ld = 34 (fp32), 36 (16-bit) / raw one element off alignment
  fuse A, B, F, Z, P, loopv                            view_pool_fuse<Px<E, T, chunk>>              E, strides % chunk == 0,
      F, D, S aligned; loopv / loop1: E / chunk (E) > 1024 * 256 (the grid cap): the stride loop runs
  fuse C (stride E + 1), D (F one element off), E37, P37 (E % chunk != 0), N65535 (E = 3), loop1 (E = 262144 + 77)   view_pool_fuse_*<1>
  ssa v64, v64o, loopv                                 scale_shift_act<Px<E, T, chunk>>             c, x_ld, y_ld % chunk == 0
      and x, y (fp32: scale, shift too) aligned; loopv: npix * c / chunk > 4096 * 256 (gv_grid_for's cap)
  ssa s6, s8_9, sc4 (fp32: scale 4 bytes off), loops   scale_shift_act_*<1>
  gap / dense / metrics                                one kernel each; blocks below, at and above a multiple of 256
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gvcnn_tf_amd import _lib                       # noqa: E402
import head_ref as HR                               # noqa: E402   (tests/head_ref.py)
from slab import DEV, NAN, SENTINEL, _Slab          # noqa: E402   (tests/slab.py)

F32 = np.float32
U = 2.0 ** -24
TYPES = {"f32": (_lib.GV_F32, torch.float32, 0.0), "bf16": (_lib.GV_BF16, torch.bfloat16, 2.0 ** -8),
         "f16": (_lib.GV_F16, torch.float16, 2.0 ** -11)}
TNAMES = list(TYPES)


def lib():
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def _chunk(tdt):
    return 16 // torch.empty(0, dtype=tdt).element_size()


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV)


def _ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g, device=DEV).float()


def _within(tag, what, got, want, bound):
    """|got - want| <= bound element by element (float64, on the device); NaN only where the reference has it.  The worst
    error / bound and the worst error relative to the tensor's scale are printed first."""
    got, want = got.double().reshape(want.shape), want.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=want.device).expand(want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s %s: NaN in other places than the reference's" % (tag, what)
    err = torch.where(nan, torch.zeros_like(want), (got - want).abs())
    fin = torch.where(nan | torch.isinf(want), torch.zeros_like(want), want.abs())
    scale = max(float(fin.max()), 1e-300)
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    print("HEAD %s | %s | err/bound %.3f | rel %.3e" % (tag, what, ratio, float(err.max()) / scale))
    assert bool((err <= bound).all()), "%s %s: error up to %.3f of its bound (%.3e of the scale)" % (
        tag, what, ratio, float(err.max()) / scale)


# ---- view_score_partial -------------------------------------------------------------------------------------------------
# name: (hw, chunks per pixel (None: cr given), cr, extra chunks of raw_ld (or elements: scalar cases), 16-byte offsets, raw base off)
SCORE_CASES = {
    "idle": (16, 8, None, 0, 0, 0), "tail3": (25, 24, None, 0, 0, 0), "trip": (32, 32, None, 0, 0, 0),
    "straddle": (49, 24, None, 0, 0, 0), "trips": (100, 50, None, 0, 0, 0), "hw1": (1, 8, None, 0, 0, 0),
    "straddle+ld1": (49, 24, None, 1, 0, 0), "tail3+ld2": (25, 24, None, 2, 0, 0), "trip+16B": (32, 32, None, 0, 1, 0),
    "trips+ld1+16B": (100, 50, None, 1, 1, 0),
    "cr30": (20, None, 30, 0, 0, 0), "ld34": (20, None, 32, "odd", 0, 0), "base1": (16, None, 32, 0, 0, 1),
}


def _score_chain(hw, cr, ld, chunk, vector):
    """Longest chain of fp32 additions of view_score_partial: the trips of thread 0 into one partial sum (unrolled trips and
    tail trips both add into sp[0]), the 4-way fold (2), 6 shuffle steps, the 4 wave partials (3)."""
    if vector:
        total, i, trips = hw * (cr // chunk), 0, 0
        while i + 3 * 256 < total:
            i, trips = i + 4 * 256, trips + 1
        while i < total:
            i, trips = i + 256, trips + 1
    else:
        trips = -(-hw * cr // 256)
    return trips + 2 + 6 + 3


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_view_score_partial_over_its_loops_and_branches(case, tname):
    """gv_view_score_partial at SCORE_CASES, N in {1, 3} x V in {1, 4, 5} x both image orders, every view with its own
    kernel row and bias.  Integers: bit for bit fl(fl(sum / hw) + bias).  Random: the fp64 bound with d = trips + 11.

    Measured worst case over the sweep, error / bound (bound: (d + 2) 2^-23 sum|terms| / hw + 2^-23 (sum|terms| / hw + |bias|)):
                        fp32      bf16      fp16
      vector walk       0.029     0.023     0.026    (relative to the tensor's scale: 3.0e-7 / 2.6e-6 / 6.3e-7)
      scalar branch     0.019     0.013     0.013    (1.8e-7 / 1.7e-7 / 1.1e-7)"""
    dt, tdt, _ = TYPES[tname]
    hw, cg, cr, extra, off16, base = SCORE_CASES[case]
    chunk = _chunk(tdt)
    cr = cr if cr is not None else cg * chunk
    ld = cr + ((2 if tname == "f32" else 4) if extra == "odd" else extra * chunk)
    o = off16 * chunk + base
    ok = off16 * 4                                                    # the kernel rows are fp32
    vector = cr % chunk == 0 and ld % chunk == 0 and base == 0
    d = _score_chain(hw, cr, ld, chunk, vector)
    for N in (1, 3):
        for V in (1, 4, 5):
            for order in (HR.SHAPE_MAJOR, HR.VIEW_MAJOR):
                nb = N * V
                g = _gen(hw, cr, N, V, order)
                tag = "score %s %s N%d V%d o%d" % (case, tname, N, V, order)
                for exact in (True, False):
                    xs = _ints(g, 4, nb * hw, cr) if exact else _randn(g, nb * hw, cr)
                    ks = _ints(g, 3, V, cr) if exact else _randn(g, V, cr) * 0.3
                    raw = _Slab(nb * hw, cr, ld, o, tdt, NAN, xs.to(tdt))
                    kern = _Slab(V, cr, cr, ok, torch.float32, NAN, ks)
                    bias = _Slab(1, V, V, 1, torch.float32, NAN, _randn(g, V))
                    out = _Slab(1, nb, nb, 3, torch.float32, SENTINEL, tail=5)
                    _lib.check(lib().gv_view_score_partial(raw.ptr, nb, hw, cr, ld, kern.ptr, bias.ptr, V, order, out.ptr,
                                                           dt, st()), tag)
                    want, sabs = HR.score_partial(raw.v.reshape(nb, hw, cr), kern.v, bias.v[0], V, order)
                    assert out.outside_intact(), tag
                    if exact:
                        assert float(sabs.max()) < 2.0 ** 24 and hw * cr < 2 ** 20
                        v = HR.view_of_image(nb, V, order)
                        s = (want - bias.v[0].double()[torch.as_tensor(v, device=DEV)]) * hw      # the integer sums
                        s = s.round().cpu().numpy().astype(F32)
                        exp = (s / F32(hw)).astype(F32) + bias.v[0].cpu().numpy()[v]
                        assert exp.dtype == F32 and out.v[0].cpu().numpy().tobytes() == exp.tobytes(), tag
                    else:
                        bound = (d + 2) * 2.0 ** -23 * sabs / hw + 2 * U * (sabs / hw + bias.v[0].double().abs()[
                            torch.as_tensor(HR.view_of_image(nb, V, order), device=DEV)])
                        _within(tag, "r_img %s" % tname, out.v[0], want, bound)


# ---- view_score_finalize, view_score_per_shape --------------------------------------------------------------------------
def _score_bound(r, want, dr=None):
    """(4 |ln r| + 6) 2^-24 relative (module docstring) + 2^-126; with an uncertainty dr of r itself (the batch mean's fp32
    sum), |d score / d r| = 1 / (1 + r)^2 at the near end and |ln r| at the far one; r within 2 dr of 0: the score is
    below r + dr."""
    r = r.double().abs()
    dr = torch.zeros_like(r) if dr is None else dr
    lo, hi = (r - dr).clamp_min(1e-300), r + dr
    ln = torch.maximum(torch.log(lo).abs(), torch.log(hi).abs())
    ln = torch.where(torch.isfinite(ln), ln, torch.zeros_like(ln))
    b = (4 * ln + 6) * U * want.abs() + 2.0 ** -126 + dr / (1 + (r - dr).clamp_min(0)) ** 2
    b = torch.where(r <= 2 * dr, torch.maximum(b, 3 * dr), b)
    return torch.where(torch.isfinite(b), b, torch.zeros_like(b))


def _special_r(n, g):
    """n responses: +-0, +-inf, NaN, subnormals, negative values, then |r| across [1e-30, 1e30] with random signs."""
    head = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), NAN, 1e-40, -3e-39, 1.1754944e-38, -2.5, 1.0, -1.0, 0.5][:n],
                        device=DEV)
    m = n - head.numel()
    rest = 10.0 ** torch.linspace(-30, 30, max(m, 1), device=DEV)[:m]
    rest = rest * (torch.randint(0, 2, (m,), generator=g, device=DEV).float() * 2 - 1)
    return torch.cat([head, rest])


def _check_special(tag, r, got):
    r, got = r.double(), got.double()
    assert bool((got[r == 0] == 0).all()), tag                       # +-0 -> exactly 0
    assert bool((got[torch.isinf(r)] == 1).all()), tag               # +-inf -> exactly 1
    assert bool(torch.isnan(got[torch.isnan(r)]).all()), tag


@pytest.mark.parametrize("order", [HR.SHAPE_MAJOR, HR.VIEW_MAJOR])
def test_view_score_finalize_over_batches_and_special_values(order):
    """gv_view_score_finalize at N in {1, 3, 300} x V in {1, 4, 64}: random responses (negative means among them; the batch
    mean is a chain of N fp32 additions and a division: dr = (N + 2) 2^-23 mean|r_img|), and at N = 1 the special values:
    r = +-0 -> 0, +-inf -> 1, NaN -> NaN, subnormals, |r| across [1e-30, 1e30].  N = 3 repeats them with the same value in
    every shape of a view except the infinities' and NaN's columns, which get them once.

    Measured worst case, error / bound: random 0.23 (3.3e-7 of the scale), special values 0.45 (6.1e-8)."""
    for N in (1, 3, 300):
        for V in (1, 4, 64):
            g = _gen(N, V, order)
            tag = "finalize N%d V%d o%d" % (N, V, order)
            for special in ((False, True) if N <= 3 else (False,)):
                if special:
                    rv = _special_r(V, g)
                    r2 = rv[None, :].repeat(N, 1)                                  # [n, v]
                    r2[1:, ~torch.isfinite(rv)] = 1.0
                    r2[1:, rv.abs() > 1e37] = 0.0                                  # the sum stays finite
                else:
                    r2 = _randn(g, N, V) * 2 + _randn(g, V)[None, :] * 0.5
                flat = (r2 if order == HR.SHAPE_MAJOR else r2.t()).reshape(-1)
                r_img = _Slab(1, N * V, N * V, 1, torch.float32, NAN, flat)
                out = _Slab(1, V, V, 3, torch.float32, SENTINEL, tail=5)
                _lib.check(lib().gv_view_score_finalize(r_img.ptr, N, V, order, out.ptr, st()), tag)
                want, mean, mabs = HR.view_score(r_img.v[0], N, V, order)
                dr = (N + 2) * 2.0 ** -23 * mabs if N > 1 else torch.zeros_like(mabs)
                dr = torch.where(torch.isfinite(dr), dr, torch.zeros_like(dr))
                _within(tag, "score %s" % ("special" if special else "random"), out.v[0], want, _score_bound(mean, want, dr))
                _check_special(tag, mean, out.v[0])
                assert out.outside_intact(), tag


@pytest.mark.parametrize("nb", [1, 257, 1000])
def test_view_score_per_shape_special_values(nb):
    """gv_view_score_per_shape at nb in {1, 257, 1000} (one, two and four workgroups, ragged): the special values of the
    finalize test, one response per image.

    Measured worst case, error / bound: 0.67 (9.0e-8 of the scale)."""
    g = _gen(nb)
    for rv in (_special_r(nb, g), _randn(g, nb) * 3):
        r_img = _Slab(1, nb, nb, 1, torch.float32, NAN, rv)
        out = _Slab(1, nb, nb, 3, torch.float32, SENTINEL, tail=5)
        _lib.check(lib().gv_view_score_per_shape(r_img.ptr, nb, out.ptr, st()), "per_shape")
        want = HR.view_score_per_shape(r_img.v[0])
        _within("per_shape nb%d" % nb, "score", out.v[0], want, _score_bound(r_img.v[0], want))
        _check_special("per_shape", r_img.v[0], out.v[0])
        assert out.outside_intact()


# ---- group_assign, group_assign_per_shape -------------------------------------------------------------------------------
def _edge_scores(num_bins):
    """k / num_bins as fp32 with its two fp32 neighbours, k = 0 .. num_bins, then NaN, 1, a negative score."""
    e = (np.arange(num_bins + 1, dtype=np.float64) / num_bins).astype(F32)
    s = np.stack([np.nextafter(e, F32(-1)), e, np.nextafter(e, F32(2))], 1).reshape(-1)
    return np.concatenate([s, np.array([np.nan, 1.0, -0.5, -1e-3, 0.999], F32)]).astype(F32)


def _assign_outputs(N, V, G):
    return (_Slab(N, V, V, 1, torch.int32, int(SENTINEL), tail=3), _Slab(N * G, V, V, 2, torch.int32, int(SENTINEL), tail=3),
            _Slab(N, G, G, 3, torch.float32, SENTINEL, tail=3), torch.full((1,), 77, dtype=torch.int32, device=DEV))


def _assign_equal(tag, outs, want, N, V, G):
    gidx, scheme, weight, status = outs
    w_gidx, w_scheme, w_weight, w_status = want
    assert int(status.item()) == w_status, (tag, int(status.item()), w_status)
    assert gidx.v.cpu().numpy().tolist() == np.asarray(w_gidx).reshape(N, V).tolist(), tag
    assert scheme.v.cpu().numpy().tolist() == np.asarray(w_scheme).reshape(N * G, V).tolist(), tag
    assert weight.v.cpu().numpy().tobytes() == np.asarray(w_weight, F32).reshape(N, G).tobytes(), tag
    assert gidx.outside_intact() and scheme.outside_intact() and weight.outside_intact(), tag


def test_group_assign_at_every_bin_edge_bit_for_bit():
    """gv_group_assign and gv_group_assign_per_shape (both weight modes) at V = 64, G = 64, num_bins = 64 on every bin edge
    k / 64 with its two fp32 neighbours and the status cases (NaN, a score of 1, negative scores), and at V = 1: gidx, scheme,
    weights and status equal the ordered restatement bit for bit (int(float32(s) * float32(64)); mean-score weights: fp32 sum
    in view order, one division, 0 for an empty group)."""
    G = B = 64
    s = _edge_scores(B)
    s = np.concatenate([s, np.full(-len(s) % 64, 0.3, F32)])
    rows = s.reshape(-1, 64)
    perm = np.random.RandomState(0).permutation(len(s))
    rows = np.concatenate([rows, s[perm].reshape(-1, 64)])                         # edges of different bins in one launch
    N = rows.shape[0]
    sd = _Slab(N, 64, 64, 1, torch.float32, NAN, torch.from_numpy(rows).to(DEV))
    for n in range(N):
        outs = _assign_outputs(1, 64, G)
        _lib.check(lib().gv_group_assign(sd.v[n].data_ptr(), 64, G, B, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                         outs[3].data_ptr(), st()), "assign")
        _assign_equal("assign row %d" % n, outs, HR.group_assign_f32(rows[n], G, B), 1, 64, G)
    for wm, name in ((_lib.GV_WEIGHT_COUNT, "count"), (_lib.GV_WEIGHT_MEAN_SCORE, "mean_score")):
        outs = _assign_outputs(N, 64, G)
        _lib.check(lib().gv_group_assign_per_shape(sd.ptr, N, 64, G, B, wm, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                   outs[3].data_ptr(), st()), "assign per shape")
        want = HR.group_assign_per_shape_f32(rows, G, B, name)
        assert (want[2] == 0).any() or name == "count"                            # empty groups under mean-score
        _assign_equal("per shape %s" % name, outs, want, N, 64, G)
        # valid scores only: status 0, and a different G / num_bins (bins beyond G are reported)
        ok = np.abs(np.random.RandomState(1).uniform(0, 0.999, size=(3, 64))).astype(F32)
        okd = torch.from_numpy(ok).to(DEV)
        for G2, B2, st_want in ((64, 64, 0), (10, 10, 0), (9, 10, 1)):
            outs = _assign_outputs(3, 64, G2)
            _lib.check(lib().gv_group_assign_per_shape(okd.data_ptr(), 3, 64, G2, B2, wm, outs[0].ptr, outs[1].ptr,
                                                       outs[2].ptr, outs[3].data_ptr(), st()), "assign per shape")
            want = HR.group_assign_per_shape_f32(ok, G2, B2, name)
            assert want[3] == st_want
            _assign_equal("per shape %s G%d" % (name, G2), outs, want, 3, 64, G2)
        # V = 1
        one = torch.tensor([[0.5], [0.984375], [0.0]], device=DEV)
        outs = _assign_outputs(3, 1, G)
        _lib.check(lib().gv_group_assign_per_shape(one.data_ptr(), 3, 1, G, B, wm, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                   outs[3].data_ptr(), st()), "assign per shape V1")
        _assign_equal("per shape V1", outs, HR.group_assign_per_shape_f32(one.cpu().numpy(), G, B, name), 3, 1, G)
    for sc in (0.5, 0.984375, float(np.nextafter(F32(0.5), F32(0)))):
        outs = _assign_outputs(1, 1, G)
        one = torch.tensor([sc], device=DEV)
        _lib.check(lib().gv_group_assign(one.data_ptr(), 1, G, B, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].data_ptr(),
                                         st()), "assign V1")
        _assign_equal("assign V1", outs, HR.group_assign_f32(one.cpu().numpy(), G, B), 1, 1, G)


def test_group_assign_entry_points_agree_and_own_the_status_word():
    """One kernel behind both entry points: on the same row gv_group_assign and gv_group_assign_per_shape (N = 1, count
    weights) give identical gidx, scheme, weight and status, at V = 64, G = 64 and at V = 1, on a clean row, a row with a NaN
    and a row with an out-of-range score.  A stale status word (3) is overwritten to 0 by a clean batch-level call and
    cleared by a clean per-shape call with N = 3."""
    G = B = 64
    clean = np.random.RandomState(2).uniform(0, 0.999, size=64).astype(F32)
    with_nan, outside = clean.copy(), clean.copy()
    with_nan[[0, 31, 63]] = np.nan
    outside[[5, 63]] = [1.0, -0.5]
    rows = [(clean, 0), (with_nan, 2), (outside, 1), (clean[:1], 0), (with_nan[:1], 2), (outside[5:6], 1)]
    for row, st_want in rows:
        V = len(row)
        sd = torch.from_numpy(row).to(DEV)
        a, b = _assign_outputs(1, V, G), _assign_outputs(1, V, G)
        _lib.check(lib().gv_group_assign(sd.data_ptr(), V, G, B, a[0].ptr, a[1].ptr, a[2].ptr, a[3].data_ptr(), st()), "assign")
        _lib.check(lib().gv_group_assign_per_shape(sd.data_ptr(), 1, V, G, B, _lib.GV_WEIGHT_COUNT, b[0].ptr, b[1].ptr,
                                                   b[2].ptr, b[3].data_ptr(), st()), "assign per shape")
        assert int(a[3].item()) == int(b[3].item()) == st_want, (V, st_want)
        for x, y in zip(a[:3], b[:3]):
            assert x.v.cpu().numpy().tobytes() == y.v.cpu().numpy().tobytes() and x.outside_intact() and y.outside_intact()
    sd = torch.from_numpy(np.stack([clean, clean[::-1], clean])).to(DEV)
    for N in (1, 3):
        outs = _assign_outputs(N, 64, G)
        outs[3].fill_(3)
        if N == 1:
            _lib.check(lib().gv_group_assign(sd.data_ptr(), 64, G, B, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                             outs[3].data_ptr(), st()), "assign")
        else:
            _lib.check(lib().gv_group_assign_per_shape(sd.data_ptr(), N, 64, G, B, _lib.GV_WEIGHT_COUNT, outs[0].ptr,
                                                       outs[1].ptr, outs[2].ptr, outs[3].data_ptr(), st()), "assign per shape")
        assert int(outs[3].item()) == 0, N


# ---- view_pool_fuse_fwd, _per_shape -------------------------------------------------------------------------------------
def _scheme_bits(G, V=64):
    """Views 31, 32 and 63 in use; a group of all 64 views; rows that overlap (view 31 in groups 0, 1 and 2); empty groups."""
    s = np.zeros((G, V), np.int32)
    s[0, [31, 32, 63]] = 1
    s[1, :] = 1
    s[2, [0, 31]] = 1
    s[3, 32] = 1
    s[5, [5, 63]] = 1
    s[G - 1, list(range(33, 64))] = 1
    return s


def _scheme_one_hot(G, V, seed):
    s = np.zeros((G, V), np.int32)
    s[np.random.RandomState(seed).randint(0, G, size=V), np.arange(V)] = 1
    return s


# name: (V, N, G, E or (chunks, extra elements), view_major, stride pad ("chunk", 1 or 0), F offset ("16B", 1 or 0), scheme, weights)
FUSE_CASES = {
    "A": (64, 3, 64, (5, 0), 0, 0, 0, "bits", "rand"),
    "B": (64, 3, 64, (5, 0), 1, "chunk", "16B", "bits", "rand"),
    "C": (64, 2, 64, (5, 0), 0, 1, 0, "bits", "rand"),
    "D": (64, 2, 64, (5, 0), 1, 0, 1, "bits", "rand"),
    "E37": (64, 2, 64, (4, 5), 0, 0, 0, "bits", "rand"),
    "F": (5, 2, 3, (2, 0), 0, 0, 0, "empty", "rand"),
    "Z": (64, 2, 64, (5, 0), 1, 0, 0, "bits", "zero_sum"),
    "P": (64, 3, 64, (5, 0), 0, "chunk", 0, "per_shape", "per_shape"),
    "P37": (64, 3, 64, (4, 5), 1, 0, 0, "per_shape", "per_shape"),
    "N65535": (2, 65535, 2, 3, 0, 0, 0, "two", "rand"),
    "loop1": (2, 1, 2, 262144 + 77, 0, 0, 0, "two", "rand"),
    "loopv": (2, 1, 2, (262144 + 19, 0), 0, 0, 0, "two", "rand"),     # fp32: E = 1 048 576 + 4 * 19, 16-bit: 2 097 152 + 8 * 19
}


def _fuse_operands(case, tname, with_outputs=True):
    dt, tdt, _ = TYPES[tname]
    V, N, G, E, view_major, pad, foff, skind, wkind = FUSE_CASES[case]
    chunk = _chunk(tdt)
    E = E if isinstance(E, int) else E[0] * chunk + E[1]
    ld = E + (chunk if pad == "chunk" else pad)
    off = chunk if foff == "16B" else foff
    g = _gen(V, N, G, E, view_major, len(case))
    vs, ss = (N * ld, ld) if view_major else (ld, V * ld)
    slab = _Slab(N * V, E, ld, off, tdt, NAN, _randn(g, N * V, E).to(tdt))
    F3 = slab.buf.as_strided((N, V, E), (ss, vs, 1), off)
    rng = np.random.RandomState(len(case) + V)
    if skind == "bits":
        scheme = _scheme_bits(G)
    elif skind == "empty":
        scheme = np.zeros((G, V), np.int32)
    elif skind == "two":
        scheme = np.array([[1, 1], [0, 1]], np.int32)                              # overlapping rows
    else:
        scheme = np.stack([_scheme_bits(G), _scheme_one_hot(G, V, 3), np.zeros((G, V), np.int32)])[:N]
    if wkind == "rand":
        weight = rng.randn(G).astype(F32)
    elif wkind == "zero_sum":
        weight = np.zeros(G, F32)
        weight[:6] = [1.5, -1.5, 2.25, -2.25, 0.0, 0.0]
    else:
        weight = rng.randn(N, G).astype(F32)
        weight[N - 1] = 0.0                                                        # mean-score weights of a shape with r = 0
    return dict(dt=dt, tdt=tdt, V=V, N=N, G=G, E=E, vs=vs, ss=ss, slab=slab, F3=F3, scheme=scheme, weight=weight,
                chunk=chunk, off=off, per_shape=scheme.ndim == 3,
                sd=torch.from_numpy(np.ascontiguousarray(scheme)).to(DEV), wd=torch.from_numpy(weight).to(DEV))


@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", list(FUSE_CASES))
def test_view_pool_fuse_bit_for_bit_against_the_ordered_restatement(case, tname, mode):
    """gv_view_pool_fuse_fwd / _per_shape at FUSE_CASES (masks with bits 31, 32 and 63, G = 64, a group of all 64 views,
    overlapping rows, empty groups and an all-empty scheme, arbitrary weights, sum w = 0 -> S exactly 0, both layouts, padded
    strides that keep and that break the 16-byte walk, a misaligned base, E % chunk != 0, the stride loop of every kernel
    form, N = 65 535) with D only, S only and both: fp32 storage equals the ordered fp32 restatement bit for bit, D and S;
    16-bit storage equals it rounded once to nearest even.  Random values, max and mean.  Every case of the sweep is bitwise
    (S was not while the compiler contracted fl(w * d) + acc into one FMA; the kernels now keep contraction off)."""
    op = _fuse_operands(case, tname)
    dt, tdt, N, V, G, E = op["dt"], op["tdt"], op["N"], op["V"], op["G"], op["E"]
    fn = lib().gv_view_pool_fuse_fwd_per_shape if op["per_shape"] else lib().gv_view_pool_fuse_fwd
    fill = 1.0 if mode == "max" else 0.25
    D32, S32 = HR.pool_fuse_f32(op["F3"].float().cpu().numpy(), op["scheme"], op["weight"], mode, fill)
    wD, wS = torch.from_numpy(D32).to(DEV).to(tdt).reshape(G * N, E), torch.from_numpy(S32).to(DEV).to(tdt)
    oo = op["off"] if op["off"] == op["chunk"] else 0                 # outputs follow a 16-byte offset, not a misaligned one
    big = E > 100000 or N > 1000
    for want_d, want_s in ((1, 1),) if big else ((1, 1), (1, 0), (0, 1)):
        D = _Slab(G * N, E, E, oo, tdt, SENTINEL, tail=2 * op["chunk"])
        S = _Slab(N, E, E, oo, tdt, SENTINEL, tail=2 * op["chunk"])
        tag = "fuse %s %s %s D%d S%d" % (case, tname, mode, want_d, want_s)
        _lib.check(fn(op["slab"].ptr, V, N, E, op["vs"], op["ss"], op["sd"].data_ptr(), G, op["wd"].data_ptr(),
                      _lib.GV_VIEWPOOL_MAX if mode == "max" else _lib.GV_VIEWPOOL_MEAN, fill, D.ptr if want_d else None,
                      S.ptr if want_s else None, dt, st()), tag)
        if want_d:
            assert torch.equal(D.v, wD), "%s: D differs in %d places" % (tag, int((D.v != wD).sum()))
        else:
            assert bool((D.buf == SENTINEL).all()), tag
        if want_s:
            assert torch.equal(S.v, wS), "%s: S differs in %d places" % (tag, int((S.v != wS).sum()))
            if FUSE_CASES[case][8] == "zero_sum":
                assert bool((S.v == 0).all()), tag
            if op["per_shape"]:
                assert bool((S.v[N - 1] == 0).all()), tag
        else:
            assert bool((S.buf == SENTINEL).all()), tag
        assert D.outside_intact() and S.outside_intact() and op["slab"].outside_intact(), tag


def test_view_pool_fuse_mean_of_small_integers_and_limits():
    """Mean pooling on integers |x| <= 4 (every sum exact): D = fl(sum / count) computed in numpy fp32 from the fp64 sums, bit
    for bit, in every storage type that holds it exactly (fp32).  N = 65 536, V = 65 and G = 65 return GV_E_UNSUPPORTED and
    write nothing."""
    V, N, G, E = 64, 2, 64, 24
    g = _gen(1)
    F = _ints(g, 4, N, V, E)
    scheme = _scheme_bits(G)
    D = _Slab(G * N, E, E, 0, torch.float32, SENTINEL, tail=8)
    sd, wd = torch.from_numpy(scheme).to(DEV), torch.ones(G, device=DEV)
    _lib.check(lib().gv_view_pool_fuse_fwd(F.data_ptr(), V, N, E, E, V * E, sd.data_ptr(), G, wd.data_ptr(),
                                           _lib.GV_VIEWPOOL_MEAN, 0.0, D.ptr, None, _lib.GV_F32, st()), "fuse ints")
    Fn = F.cpu().numpy().astype(np.float64)
    for gi in range(G):
        idx = np.nonzero(scheme[gi])[0]
        exp = (Fn[:, idx].sum(1).astype(F32) / F32(idx.size)).astype(F32) if idx.size else np.zeros((N, E), F32)
        assert D.v.reshape(G, N, E)[gi].cpu().numpy().tobytes() == exp.tobytes(), gi
    S = _Slab(4, 3, 3, 0, torch.float32, SENTINEL)
    small = torch.zeros(65 * 65, dtype=torch.int32, device=DEV)
    for Vx, Nx, Gx in ((2, 65536, 2), (65, 1, 2), (2, 1, 65)):
        for fn in (lib().gv_view_pool_fuse_fwd, lib().gv_view_pool_fuse_fwd_per_shape):
            rc = fn(F.data_ptr(), Vx, Nx, 3, 3, Vx * 3, small.data_ptr(), Gx, wd.data_ptr(), 0, 1.0, None, S.ptr, _lib.GV_F32, st())
            assert rc == _lib.GV_E_UNSUPPORTED, (Vx, Nx, Gx, rc)
    assert bool((S.buf == SENTINEL).all())


# ---- view_pool_fuse_bwd_t -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", ["A", "P", "loop1"])
def test_view_pool_fuse_backward_over_the_mask_edges(case, tname, mode):
    """gv_view_pool_fuse_bwd_t shares the mask code of the forward: the masks with bits 31, 32 and 63, the group of all 64
    views and the overlapping rows (A; P: per shape, one shape without weights), and the stride loop (E = 262 144 + 77),
    against fp64 autograd through the reference's forward.  fp32: 1e-5 of the tensor's scale; 16-bit dF: one rounding of the
    storage type, 2^-8 / 2^-11 of the scale (dF starts at 0).  The kernel adds every group's share into the stored dF, so a
    view that k rows of the scheme name is rounded k times: A and P, whose rows overlap, stay inside ONE rounding on their
    values; the stride-loop case has disjoint rows (with the overlapping rows [[1, 1], [0, 1]] at that E the fp16 max case
    measured 1.06 of one rounding, two roundings being what the accumulation into 16-bit storage allows).

    Measured worst case, relative to the tensor's scale:   fp32 2.2e-7 (1e-5)   bf16 2.6e-3 (3.9e-3)   fp16 4.0e-4 (4.9e-4)"""
    op = _fuse_operands(case, tname)
    dt, tdt, N, V, G, E = op["dt"], op["tdt"], op["N"], op["V"], op["G"], op["E"]
    if case == "loop1":                                               # disjoint rows: every dF element is written once
        op["scheme"] = np.array([[1, 1], [0, 0]], np.int32)
        op["sd"] = torch.from_numpy(op["scheme"]).to(DEV)
    g = _gen(E, V, 5)
    Fc = op["F3"].contiguous()                                        # [N, V, E] dense: dF has the strides of F
    dS = _Slab(N, E, E, 1, torch.float32, NAN, _randn(g, N, E))
    dF = _Slab(N * V, E, E, op["chunk"], tdt, SENTINEL, torch.zeros(N * V, E, device=DEV).to(tdt), tail=16)
    if op["per_shape"]:
        op["wd"][N - 1] = 0.0
        op["wd"][0].abs_()                                            # a sum of weights away from 0
    Fr = Fc.double().requires_grad_(True)
    _, S = HR.pool_fuse(Fr, op["scheme"], op["wd"].cpu().numpy(), mode, 1.0)
    S.backward(dS.v.double())
    tag = "fuse bwd %s %s %s" % (case, tname, mode)
    _lib.check(lib().gv_view_pool_fuse_bwd_t(Fc.data_ptr(), dS.ptr, V, N, E, E, V * E, op["sd"].data_ptr(), G,
                                             op["wd"].data_ptr(), 0 if mode == "max" else 1, dF.ptr, int(op["per_shape"]),
                                             dt, st()), tag)
    tol = 1e-5 if tname == "f32" else TYPES[tname][2]
    want = Fr.grad.reshape(N * V, E)
    _within(tag, "dF %s" % tname, dF.v, want, tol * float(want.abs().max()))
    assert dF.outside_intact() and dS.outside_intact(), tag


# ---- the four readers of one group table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("E", [8, 9])                                 # the vector and the scalar walk
def test_a_shape_whose_weights_sum_to_zero_in_every_reader_of_the_group_table(E, mode):
    """Per-shape grouping with mean_score weights, N = 2, V = 3, G = 4: every score of shape 0 is 0, so its weights sum to 0;
    shape 1 is an ordinary one.  The forward, its backward, the weight gradient and explain each load the group table of
    their shape and must agree on shape 0: S = 0, dF untouched, dw = 0, maps and view_contrib 0 with baseline = bias[k].
    Shape 1: S equals the ordered fp32 restatement bit for bit, dF is within 1e-5 of the tensor's scale of fp64 autograd,
    dw within 1e-5 of its absolute-term sum (scorer_ref.group_weight_grad), explain within (n + 8) 2^-24 of its
    absolute-term sum (explain_ref)."""
    import explain_ref as XR                                          # tests/explain_ref.py
    import scorer_ref as SR                                           # tests/scorer_ref.py
    N, V, G, nc = 2, 3, 4, 5
    pm = _lib.GV_VIEWPOOL_MAX if mode == "max" else _lib.GV_VIEWPOOL_MEAN
    g = _gen(E, N, V, G)
    scores = torch.tensor([[0.0, 0.0, 0.0], [0.15, 0.17, 0.62]], device=DEV)
    gidx, scheme, weight, status = (torch.empty(N, V, dtype=torch.int32, device=DEV),
                                    torch.empty(N, G, V, dtype=torch.int32, device=DEV), torch.empty(N, G, device=DEV),
                                    torch.zeros(1, dtype=torch.int32, device=DEV))
    _lib.check(lib().gv_group_assign_per_shape(scores.data_ptr(), N, V, G, G, _lib.GV_WEIGHT_MEAN_SCORE, gidx.data_ptr(),
                                               scheme.data_ptr(), weight.data_ptr(), status.data_ptr(), st()), "assign")
    sch, wt = scheme.cpu().numpy(), weight.cpu().numpy()
    assert int(status.item()) == 0 and not wt[0].any() and sch[0, 0].all() and float(wt[1].sum()) > 0
    F, dS = _randn(g, N, V, E), _randn(g, N, E)
    S = torch.full((N, E), SENTINEL, device=DEV)
    _lib.check(lib().gv_view_pool_fuse_fwd_per_shape(F.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(), G, weight.data_ptr(),
                                                     pm, 1.0, None, S.data_ptr(), _lib.GV_F32, st()), "fuse")
    _, S32 = HR.pool_fuse_f32(F.cpu().numpy(), sch, wt, mode, 1.0)
    assert not S[0].any() and S[1].cpu().numpy().tobytes() == S32[1].tobytes() and S32[1].any()
    dF0 = _randn(g, N, V, E)
    dF = dF0.clone()
    _lib.check(lib().gv_view_pool_fuse_bwd_t(F.data_ptr(), dS.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(), G,
                                             weight.data_ptr(), pm, dF.data_ptr(), 1, _lib.GV_F32, st()), "fuse bwd")
    Fr = F.double().requires_grad_(True)
    HR.pool_fuse(Fr, sch, wt, mode, 1.0)[1].backward(dS.double())
    assert torch.equal(dF[0], dF0[0])
    _within("zero-sum", "dF of shape 1", dF[1] - dF0[1], Fr.grad[1], 1e-5 * float(Fr.grad[1].abs().max()))
    nws = lib().gv_group_weight_bwd_workspace_bytes(N, E, G)
    ws, dw = torch.full((nws // 4,), SENTINEL, device=DEV), torch.full((N, G), SENTINEL, device=DEV)
    _lib.check(lib().gv_group_weight_bwd_per_shape(F.data_ptr(), dS.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(), G,
                                                   weight.data_ptr(), pm, dw.data_ptr(), ws.data_ptr(), nws, _lib.GV_F32, st()),
               "group_weight_bwd")
    ref, A = SR.group_weight_grad(F.cpu().double(), dS.cpu().double(), gidx.cpu(), weight.cpu().double(), G, mode)
    assert not dw[0].any() and float(dw[1].abs().max()) > 0
    assert bool(((dw[1].cpu().double() - ref[1]).abs() <= 1e-5 * A[1]).all()), (dw[1], ref[1])
    K, b, tg = _randn(g, E, nc), _randn(g, nc), np.array([1, 3])
    import gvcnn_tf_amd as gv
    for kind in ("exact", "gradcam"):
        ex = gv.explain_views(F.reshape(N, V, 1, 1, E), scheme, weight, K, b, target=tg, pool=mode, empty_fill=1.0, kind=kind)
        want = XR.explain(F.cpu().numpy().reshape(N, V, 1, E), sch, wt, K.cpu().numpy(), b.cpu().numpy(), tg, mode, 1.0, kind)
        got = dict(maps=ex.maps.reshape(N, V, 1), view_contrib=ex.view_contrib, baseline=ex.baseline)
        assert not got["maps"][0].any() and not got["view_contrib"][0].any() and float(ex.baseline[0]) == float(b[tg[0]])
        for name, t in got.items():
            val, n, T = (x[1] for x in want[name])
            err = np.abs(t[1].cpu().numpy().astype(np.float64) - val)
            assert (err <= 1.01 * (n + 8) * U * T).all(), (kind, name, err, T)
        assert kind == "gradcam" or got["maps"][1].any()          # (gradcam clips at 0: a single pixel may well be 0)


# ---- scale_shift_act ----------------------------------------------------------------------------------------------------
# name: (npix, c or chunks, x_ld - c, y_ld - c, 16-byte offsets, scale offset in elements); "k" widths are in chunks
SSA_CASES = {
    "v64": (37, 64, 0, 8, 0, 0), "v64o": (37, 64, 8, 0, 1, 0), "s6": (37, 6, 0, 2, 0, 0), "s8_9": (37, 8, 1, 1, 0, 0),
    "sc4": (37, 64, 0, 0, 0, 1), "loopv": (4096 * 256 + 3, "chunk", 0, 0, 0, 0), "loops": (4096 * 256 + 3, 1, 0, 0, 0, 0),
}


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", list(SSA_CASES))
def test_scale_shift_act_vector_and_scalar_forms(case, tname):
    """gv_scale_shift_act at SSA_CASES with relu 0 and 1: integers bit for bit; random values within two fp32 roundings of
    x * scale + shift (one if the compiler fuses them: 2 * 2^-24 (|x scale| + |shift|)) plus the storage type's rounding.
    sc4 (a scale pointer 4 bytes off alignment) selects the scalar kernel on fp32 storage only; the 16-bit kernels read the
    coefficients one by one.

    Measured worst case:  fp32 error / bound 0.50 (one rounding: the compiler fuses), 4.4e-8 of the scale;  bf16 2.8e-3 of
    the scale (3.9e-3);  fp16 4.5e-4 (4.9e-4)"""
    dt, tdt, eps = TYPES[tname]
    npix, c, dx, dy, off16, soff = SSA_CASES[case]
    chunk = _chunk(tdt)
    c = chunk if c == "chunk" else c
    o = off16 * chunk
    g = _gen(npix, c, dx, dy, soff)
    for exact in ((False,) if npix > 1000 else (True, False)):
        xs = _ints(g, 4, npix, c) if exact else _randn(g, npix, c)
        sc = _Slab(1, c, c, soff, torch.float32, NAN, _ints(g, 3, c) if exact else torch.rand(c, generator=g, device=DEV) + 0.5)
        sh = _Slab(1, c, c, soff, torch.float32, NAN, _ints(g, 3, c) if exact else _randn(g, c))
        x = _Slab(npix, c, c + dx, o, tdt, NAN, xs.to(tdt))
        for relu in (0, 1):
            y = _Slab(npix, c, c + dy, o, tdt, SENTINEL, tail=2 * chunk)
            tag = "ssa %s %s relu%d" % (case, tname, relu)
            _lib.check(lib().gv_scale_shift_act(x.ptr, npix, c, c + dx, sc.ptr, sh.ptr, relu, y.ptr, c + dy, dt, st()), tag)
            want, mag = HR.scale_shift_act(x.v, sc.v[0], sh.v[0], relu)
            if exact:
                assert torch.equal(y.v.double(), want), tag
            else:
                _within(tag, "y %s" % tname, y.v, want, 2 * U * mag + eps * float(want.abs().max()))
            assert y.outside_intact(), tag
        assert x.outside_intact()


# ---- global_avg_pool ----------------------------------------------------------------------------------------------------
GAP_CASES = [(12, 49, 20, 20), (256, 1, 1, 1), (13, 49, 20, 28), (1, 1225, 2048, 2048), (3, 1225, 1, 3), (1, 1, 2048, 2056),
             (257, 49, 1, 1), (5, 49, 20, 24)]


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("nb,hw,c,ld", GAP_CASES)
def test_global_avg_pool_over_maps_channels_and_blocks(nb, hw, c, ld, tname):
    """gv_global_avg_pool at hw in {1, 49, 1225}, c in {1, 20, 2048}, x_ld > c, nb * c below (240, 100), at (256, 2048) and
    above (257, 260) a multiple of 256.  Integers: fl(sum / hw) bit for bit.  Random: d = hw additions and the division.

    Measured worst case, error / bound ((hw + 2) 2^-23 sum|x| / hw + 2^-24 sum|x| / hw):  fp32 0.024  bf16 0.004  fp16 0.003
    (relative to the tensor's scale: 1.0e-6 / 9.6e-8 / 1.0e-7)"""
    dt, tdt, _ = TYPES[tname]
    g = _gen(nb, hw, c, ld)
    for exact in (True, False):
        xs = _ints(g, 4, nb * hw, c) if exact else _randn(g, nb * hw, c)
        x = _Slab(nb * hw, c, ld, _chunk(tdt), tdt, NAN, xs.to(tdt))
        y = _Slab(nb, c, c, 3, torch.float32, SENTINEL, tail=5)
        tag = "gap %dx%dx%d/%d %s" % (nb, hw, c, ld, tname)
        _lib.check(lib().gv_global_avg_pool(x.ptr, nb, hw, c, ld, y.ptr, dt, st()), tag)
        want, sabs = HR.global_avg_pool(x.v.reshape(nb, hw, c))
        if exact:
            assert float(sabs.max()) < 2.0 ** 24 and hw < 2 ** 20
            exp = ((want * hw).round().cpu().numpy().astype(F32) / F32(hw)).astype(F32)
            assert y.v.cpu().numpy().tobytes() == exp.tobytes(), tag
        else:
            _within(tag, "gap %s" % tname, y.v, want, (hw + 2) * 2.0 ** -23 * sabs / hw + U * sabs / hw)
        assert y.outside_intact() and x.outside_intact(), tag


# ---- dense_fwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 24, 255, 256, 2048, 2049])
def test_dense_over_feature_counts(f):
    """gv_dense_fwd at f in {1, 24, 255, 256, 2048, 2049} (idle lanes, a full block, a ragged last trip) x c in {1, 40} x
    n in {1, 5}.  Integers: sum + bias bit for bit.  Random: d = ceil(f / 256) trips + 6 shuffle steps + the 4 wave partials
    and the bias (4).  c = 65 536 returns GV_E_UNSUPPORTED.

    Measured worst case, error / bound ((d + 2) 2^-23 (sum|x k| + |bias|)): 0.040 (7.3e-7 of the tensor's scale)"""
    d = -(-f // 256) + 6 + 4
    for c in (1, 40):
        for n in (1, 5):
            g = _gen(f, c, n)
            for exact in (True, False):
                x = _Slab(n, f, f, 1, torch.float32, NAN, _ints(g, 4, n, f) if exact else _randn(g, n, f))
                k = _Slab(f, c, c, 3, torch.float32, NAN, _ints(g, 3, f, c) if exact else _randn(g, f, c) * 0.05)
                b = _Slab(1, c, c, 1, torch.float32, NAN, _ints(g, 3, c) if exact else _randn(g, c))
                y = _Slab(n, c, c, 3, torch.float32, SENTINEL, tail=5)
                tag = "dense f%d c%d n%d" % (f, c, n)
                _lib.check(lib().gv_dense_fwd(x.ptr, n, f, k.ptr, b.ptr, c, y.ptr, st()), tag)
                want, sabs = HR.dense(x.v, k.v, b.v[0])
                if exact:
                    assert float(sabs.max()) < 2.0 ** 24 and f < 2 ** 20
                    assert torch.equal(y.v.double(), want), tag
                else:
                    _within(tag, "dense", y.v, want, (d + 2) * 2.0 ** -23 * sabs)
                assert y.outside_intact(), tag
    y = _Slab(1, 4, 4, 0, torch.float32, SENTINEL)
    assert lib().gv_dense_fwd(y.ptr, 1, 1, y.ptr, y.ptr, 65536, y.ptr, st()) == _lib.GV_E_UNSUPPORTED
    assert bool((y.buf == SENTINEL).all())


# ---- eval_metrics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 40])
def test_eval_metrics_accumulates_over_several_workgroups(c):
    """gv_eval_metrics at n = 300 (three workgroups of 128, the last ragged), c in {1, 2, 40} (c = 2: many shapes on one
    confusion cell), ties (logits are small integers: the first maximum wins), labels -1 and c (counted nowhere), confusion
    and correct starting non-zero (the contract is accumulate).  NaN logits are NOT pinned by this test: `>` against a NaN
    is false, so the kernel's answer depends on where the NaN stands, and eval.py's argmax has no contract for it either."""
    n = 300
    rng = np.random.RandomState(c)
    logits = rng.randint(-2, 3, size=(n, c)).astype(F32)
    labels = rng.randint(-1, c + 1, size=n).astype(np.int64)
    assert (labels == -1).any() and (labels == c).any() and (c == 1 or (np.sort(logits, 1)[:, -1] == np.sort(logits, 1)[:, -2]).any())
    conf0 = rng.randint(0, 5, size=(c, c)).astype(np.int32)
    ld = _Slab(n, c, c, 1, torch.float32, NAN, torch.from_numpy(logits).to(DEV))
    lab = torch.from_numpy(labels).to(DEV)
    pred = _Slab(1, n, n, 1, torch.int64, int(SENTINEL), tail=3)
    conf = _Slab(c, c, c, 1, torch.int32, int(SENTINEL), torch.from_numpy(conf0).to(DEV), tail=3)
    corr = torch.tensor([11], dtype=torch.int32, device=DEV)
    for rounds in (1, 2):
        _lib.check(lib().gv_eval_metrics(ld.ptr, lab.data_ptr(), n, c, pred.ptr, conf.ptr, corr.data_ptr(), st()), "eval")
        w_pred, w_conf, w_corr = HR.eval_metrics(logits, labels, conf0, 11)
        for _ in range(rounds - 1):
            w_pred, w_conf, w_corr = HR.eval_metrics(logits, labels, w_conf, w_corr)
        assert pred.v[0].cpu().numpy().tolist() == w_pred.tolist()
        assert conf.v.cpu().numpy().tolist() == w_conf.tolist() and int(corr.item()) == w_corr
        assert pred.outside_intact() and conf.outside_intact()
