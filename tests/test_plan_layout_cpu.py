"""The pure arithmetic of the inference plan builder (gvcnn-tf_amd/_plan_layout.py): buffer assignment and lane
dependencies against a replay and a brute-force restatement written here, arena offsets, ResNet unit forms and flag words
against literals read from the plans of the commit that introduced the module, the autotuner's selection rules.
The module is loaded from its file: no device, no library."""
import importlib.util
import os
import random
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gv_plan_layout", os.path.join(ROOT, "gvcnn-tf_amd", "_plan_layout.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)

R, W = False, True


def full(v, w, c=16):
    """One access to the whole of a c-channel tensor."""
    return (v, w, 0, c)


def plain(*sizes):
    return [[n, False, False] for n in sizes]


# ---- buffer assignment ---------------------------------------------------------------------------
def test_a_lane_reuses_its_own_buffer_at_once():
    acc = [[full(0, W)], [full(0, R), full(1, W)], [full(1, R), full(2, W)]]
    vmap, sizes, fmts = L.assign_buffers(acc, [0, 0, 0], plain(100, 100, 100), 16)
    assert vmap == {0: 0, 1: 1, 2: 0} and sizes == [100, 100] and fmts == [False, False]


@pytest.mark.parametrize("gap,reused", [(15, False), (16, True)])
def test_another_lane_waits_sixteen_ops_for_a_freed_buffer(gap, reused):
    """Released by lane 0 at op 1; lane 1 asks at op 1 + gap."""
    acc = [[full(0, W)], [full(0, R)]] + [[] for _ in range(gap - 1)] + [[full(1, W)]]
    lanes = [0, 0] + [1] * gap
    vmap, sizes, _ = L.assign_buffers(acc, lanes, plain(100, 100), L.REUSE_DELAY)
    assert (vmap[1] == vmap[0]) == reused and len(sizes) == (1 if reused else 2)
    # ... the releasing lane itself does not wait, and without lanes nobody does
    assert L.assign_buffers(acc, [0] * len(acc), plain(100, 100), 16)[0] == {0: 0, 1: 0}
    assert L.assign_buffers(acc[:2] + acc[-1:], [0, 0, 1], plain(100, 100), 0)[0] == {0: 0, 1: 0}


def test_the_biggest_reusable_buffer_is_enlarged_where_none_fits():
    acc = [[full(0, W)], [full(1, W)], [full(0, R), full(1, R)], [full(2, W)], [full(3, W)]]
    vmap, sizes, _ = L.assign_buffers(acc, [0] * 5, plain(10, 20, 30, 5), 16)
    assert vmap == {0: 0, 1: 1, 2: 1, 3: 0} and sizes == [10, 30]          # no third buffer; the small one serves the small tensor
    # the smallest buffer that fits is taken
    vmap, sizes, _ = L.assign_buffers(acc, [0] * 5, plain(10, 20, 8, 15), 16)
    assert vmap == {0: 0, 1: 1, 2: 0, 3: 1} and sizes == [10, 20]


def test_plain_and_three_plane_tensors_never_share_a_buffer():
    acc = [[full(0, W)], [full(0, R)], [full(1, W)], [full(1, R)], [full(2, W)], [full(3, W)]]
    vbufs = [[100, False, False], [50, False, True], [50, False, False], [50, False, True]]
    vmap, sizes, fmts = L.assign_buffers(acc, [0] * 6, vbufs, 16)
    assert vmap == {0: 0, 1: 1, 2: 0, 3: 1} and fmts == [False, True] and sizes == [100, 50]
    for v, p in vmap.items():
        assert fmts[p] == vbufs[v][2]


def test_a_kept_tensor_is_never_released():
    acc = [[full(0, W)], [full(0, R), full(1, W)], [full(1, R), full(2, W)], [full(2, R), full(3, W)]]
    vbufs = plain(100, 100, 100, 100)
    vbufs[0][1] = True
    vmap, sizes, _ = L.assign_buffers(acc, [0] * 4, vbufs, 0)
    assert all(vmap[v] != vmap[0] for v in (1, 2, 3)) and vmap[3] == vmap[1]


def random_plan(seed):
    """An op list over 3 lanes: every op reads up to two tensors written before (whole, or one written slice) and writes a
    new tensor or the next 16-channel slice of an open concat tensor; some tensors are kept, some are three-plane."""
    rng = random.Random(seed)
    vbufs, acc, lanes, written, concat = [], [], [], [], None      # written: (vbuf, lo, hi); concat: [vbuf, next lo, ld]
    for i in range(rng.randint(20, 60)):
        a = []
        for v, lo, hi in rng.sample(written, min(len(written), rng.randint(0, 2))):
            a.append((v, R, lo, hi))
        if concat is not None and rng.random() < 0.6:
            v, lo, ld = concat
            out = (v, lo, lo + 16)
            concat = [v, lo + 16, ld] if lo + 32 <= ld else None
        else:
            ld = rng.choice((16, 32, 48, 64))
            vbufs.append([rng.choice((100, 200, 300)) * ld, rng.random() < 0.1, rng.random() < 0.25])
            v = len(vbufs) - 1
            if ld > 16 and concat is None and rng.random() < 0.5:
                out, concat = (v, 0, 16), [v, 16, ld]
            else:
                out = (v, 0, ld)
        a = [r for r in a if r[0] != out[0]]                   # (no op reads the tensor it writes)
        a.append((out[0], W, out[1], out[2]))
        written.append(out)
        acc.append(a)
        lanes.append(rng.randrange(3))
    return acc, lanes, vbufs


RANDOM_PLANS = [(seed, L.REUSE_DELAY if seed % 2 else 0) + random_plan(seed) for seed in range(200)]


def test_no_write_lands_on_a_tensor_with_a_later_read():
    shared = 0
    for seed, delay, acc, lanes, vbufs in RANDOM_PLANS:
        vmap, sizes, fmts = L.assign_buffers(acc, lanes, vbufs, delay)
        last_read = {}
        for i, a in enumerate(acc):
            for v, w, _, _ in a:
                if not w:
                    last_read[v] = i
        owner = {}
        for i, a in enumerate(acc):
            for v, w, _, _ in a:
                p = vmap[v]
                assert sizes[p] >= vbufs[v][0], (seed, i)
                assert fmts[p] == vbufs[v][2], (seed, i)
                if not w:
                    assert owner.get(p) == v, (seed, i, "reads a recycled buffer")
                    continue
                prev = owner.get(p)
                if prev is not None and prev != v:
                    assert not vbufs[prev][1], (seed, i, "overwrites a kept tensor")
                    assert last_read.get(prev, -1) < i, (seed, i, "overwrites a live tensor")
                    shared += 1
                owner[p] = v
            ins = {vmap[v] for v, w, _, _ in a if not w}
            assert not ins & {vmap[v] for v, w, _, _ in a if w}, (seed, i)
    assert shared > 1000                           # reuse happens: the check is not vacuous


# ---- lane dependencies ---------------------------------------------------------------------------
def conflicts(a, b, vmap):
    """Do two access lists conflict?  Same physical buffer, a write involved, not two disjoint slices of one tensor."""
    for vi, wi, li, hi in a:
        for vj, wj, lj, hj in b:
            if vmap[vi] == vmap[vj] and (wi or wj) and not (vi == vj and (hi <= lj or hj <= li)):
                return True
    return False


def happens_before(lanes, deps):
    """hb[i]: the ops complete before op i starts, from stream order on each lane plus the recorded dependencies."""
    hb, last = [], {}
    for i, lane in enumerate(lanes):
        s = set()
        for j in ([last[lane]] if lane in last else []) + list(deps[i]):
            s |= hb[j] | {j}
        hb.append(s)
        last[lane] = i
    return hb


def test_lane_dependencies_order_every_conflict_and_nothing_is_redundant():
    n_cross = n_deps = 0
    for seed, delay, acc, lanes, vbufs in RANDOM_PLANS:
        vmap = L.assign_buffers(acc, lanes, vbufs, delay)[0]
        deps = L.lane_deps(acc, lanes, vmap)
        hb = happens_before(lanes, deps)
        for i in range(len(acc)):
            assert all(d < i and lanes[d] != lanes[i] for d in deps[i]) and deps[i] == sorted(set(deps[i])), (seed, i)
            need = {j for j in range(i) if conflicts(acc[i], acc[j], vmap)}
            assert need <= hb[i], (seed, i, sorted(need - hb[i]))
            n_cross += sum(lanes[j] != lanes[i] for j in need)
            # the restatement: latest conflicting op first, skip what is already known to be complete
            same = [j for j in range(i) if lanes[j] == lanes[i]]
            known = hb[same[-1]] | {same[-1]} if same else set()
            want = []
            for j in sorted(need, reverse=True):
                if j not in known:
                    want.append(j)
                    known |= hb[j] | {j}
            assert deps[i] == sorted(want), (seed, i)
            n_deps += len(want)
    assert n_cross > 2000 and n_deps > 500          # not vacuous


def test_slices_of_one_tensor_are_independent_and_tensors_sharing_a_buffer_are_not():
    lanes = [0, 1, 2]
    acc = [[(0, W, 0, 16)], [(0, W, 16, 32)], [(0, R, 0, 16)]]
    assert L.lane_deps(acc, lanes, {0: 0}) == [[], [], [0]]                   # the reader waits for its slice's writer only
    acc = [[(0, W, 0, 16)], [(1, W, 16, 32)], [(0, W, 8, 24)]]
    assert L.lane_deps(acc, lanes, {0: 0, 1: 0}) == [[], [0], [1]]            # two tensors in one buffer; ([1] implies 0)
    assert L.lane_deps(acc, lanes, {0: 0, 1: 1}) == [[], [], [0]]             # ... in two; overlapping slices of one conflict
    assert L.lane_deps([[(0, W, 0, 16)], [(0, R, 0, 16)], [(0, R, 0, 16)]], lanes, {0: 0}) == [[], [0], [0]]   # reads do not


def test_accesses_of_an_op_record():
    T = lambda vbuf, off, c, ld: SimpleNamespace(vbuf=vbuf, off=off, c=c, ld=ld)
    op = dict(x=T(-1, 0, 3, 3), y=T(4, 2 * 64 + 16, 32, 64), y2=T(5, 0, 8, 8), res=T(3, 7 * 24 + 8, 16, 24), other=1)
    assert L.accesses(op) == [(3, R, 8, 24), (4, W, 16, 48), (5, W, 0, 8)]
    assert L.accesses(dict(x=T(2, 0, 8, 8), y=T(6, 0, 8, 8), y2=None)) == [(2, R, 0, 8), (6, W, 0, 8)]


# ---- arenas --------------------------------------------------------------------------------------
def test_arena_offsets_of_a_sibling_group_and_a_resnet_pair():
    """Mixed_5b's four 1x1 filters over 192 channels (fp32 plan) and block2's conv1 + projection pair (bf16 plan): the
    arena sizes in front of them, the packed sizes and the expected offsets are read from those plans."""
    s = "InceptionV3/Mixed_5b/"
    names = [s + "Branch_0/Conv2d_0a_1x1", s + "Branch_1/Conv2d_0a_1x1", s + "Branch_2/Conv2d_0a_1x1", s + "Branch_3/Conv2d_0b_1x1"]
    couts, packed = (64, 48, 64, 32), (12288, 9216, 12288, 6144)
    filters = []
    off, w_elems = L.place_filters(filters, 175104, [(n + "/weights", 1, 1, 192, c, k) for n, c, k in zip(names, couts, packed)])
    assert (off, w_elems) == (175104, 215040) and [f[5] for f in filters] == [175104, 187392, 196608, 208896]
    assert filters[1] == (names[1] + "/weights", 1, 1, 192, 48, 187392)
    specs = []
    so, ho, ss_elems = L.place_scale_shift(specs, 800, [("bn", n + "/BatchNorm", c, 0.001, False) for n, c in zip(names, couts)])
    assert (so, ho, ss_elems) == (800, 1008, 1216)
    assert [(sp[5], sp[6]) for sp in specs] == [(800, 1008), (864, 1072), (912, 1120), (976, 1184)]
    assert specs[3] == ("bn", names[3] + "/BatchNorm", 32, 0.001, False, 976, 1184)

    u = "resnet_v2_50/block2/unit_1/bottleneck_v2/"
    filters, specs = [], []
    off, w_elems = L.place_filters(filters, 111616, [(u + "conv1/weights", 1, 1, 256, 128, 16384),
                                                     (u + "shortcut/weights", 1, 1, 256, 512, 65536)])
    assert (off, w_elems) == (111616, 193536) and [f[5] for f in filters] == [111616, 128000]
    so, ho, ss_elems = L.place_scale_shift(specs, 4096, [("bn", u + "conv1/BatchNorm", 128, 1e-5, True),
                                                         ("bias", u + "shortcut/biases", 512, 0.0, False)])
    assert (so, ho, ss_elems) == (4096, 4736, 5376) and [(sp[5], sp[6]) for sp in specs] == [(4096, 4736), (4224, 4864)]
    # the roundings: a group's end to 64 units, a scale / shift row to 4 channels
    assert L.place_filters([], 64, [("a", 1, 1, 3, 5, 15), ("b", 1, 1, 3, 5, 15)]) == (64, 128)
    assert L.place_filters([], 64, [("a", 1, 1, 3, 5, 64)]) == (64, 128)
    assert L.place_scale_shift([], 8, [("bias", "a", 5, 0.0, False)]) == (8, 16, 24)
    assert L.place_scale_shift([], 8, [("bias", "a", 5, 0.0, False), ("bias", "b", 4, 0.0, False)]) == (8, 20, 32)


# ---- ResNet unit forms ---------------------------------------------------------------------------
UNITS = [(b, base, u, n, s if u == n - 1 else 1) for b, base, n, s in
         (("block1", 64, 3, 2), ("block2", 128, 4, 2), ("block3", 256, 6, 2), ("block4", 512, 3, 1)) for u in range(n)]
TAIL34 = ([("pair", "deferred")] + [("identity", "deferred")] * 4 + [("subsampled", "stored")] +
          [("pair", "stored"), ("identity", "stored"), ("identity", "last")])
BF16 = dict(lowp=True, proj0=True, fuse_chain=True, fuse_unit=True, fuse_pair=True, defer_preact=True)


def test_resnet_unit_forms_of_the_default_16bit_plan():
    assert L.resnet_unit_forms(UNITS, **BF16) == [
        ("in_gemm", "chain_proj"), ("identity", "unit"), ("subsampled", "stored"),
        ("pair", "chain"), ("identity", "chain"), ("identity", "chain"), ("subsampled", "stored")] + TAIL34
    assert len(UNITS) == 16


def test_resnet_unit_forms_under_the_switches():
    assert L.resnet_unit_forms(UNITS, **dict(BF16, fuse_unit="all")) == [
        ("in_gemm", "chain_proj"), ("identity", "unit"), ("subsampled", "stored"),
        ("pair", "unit"), ("identity", "unit"), ("identity", "unit"), ("subsampled", "stored")] + TAIL34
    # make_plan(fuse_chain=False): no chain, unit, projection-in-GEMM or pair
    off = dict(BF16, proj0=False, fuse_chain=False, fuse_unit=False, fuse_pair=False)
    block = lambda n, tail: [("conv", tail)] + [("identity", tail)] * (n - 2) + [("subsampled", "stored")]
    assert L.resnet_unit_forms(UNITS, **off) == block(3, "deferred") + block(4, "deferred") + block(6, "deferred") + [
        ("conv", "stored"), ("identity", "stored"), ("identity", "last")]
    # fp32 storage: every switch resolves to off
    f32 = dict(lowp=False, proj0=False, fuse_chain=False, fuse_unit=False, fuse_pair=False, defer_preact=False)
    assert L.resnet_unit_forms(UNITS, **f32) == block(3, "stored") + block(4, "stored") + block(6, "stored") + [
        ("conv", "stored"), ("identity", "stored"), ("identity", "last")]
    # ... and asking for them under fp32 storage changes nothing: the chain kernels are 16-bit
    assert L.resnet_unit_forms(UNITS, **dict(BF16, lowp=False, proj0=False, defer_preact=False))[:2] == [("conv", "stored"), ("identity", "stored")]


def test_block1_pair_is_not_fused_and_block4_is_never_deferred():
    forms = L.resnet_unit_forms(UNITS, **dict(BF16, proj0=False))
    assert forms[0] == ("conv", "unit")                        # base 64 < 128: conv1 and the projection stay two launches
    assert [f[0] for f in forms].count("pair") == 3
    for kw in (BF16, dict(BF16, fuse_chain=False, fuse_unit=False, proj0=False)):
        assert all(t in ("stored", "last") for _, t in L.resnet_unit_forms(UNITS, **kw)[13:])    # depth 2048 > 1024
    assert L.resnet_unit_forms(UNITS, **dict(BF16, defer_preact=False))[7:13] == [("pair", "stored")] + [("identity", "stored")] * 4 + [
        ("subsampled", "stored")]


# ---- flags and predicates ------------------------------------------------------------------------
F = SimpleNamespace(GV_CONV_RELU=1, GV_CONV_RELU2=2, GV_CONV_SPLIT=4, GV_CONV_X_F32=8, GV_CONV_X_P3=16, GV_CONV_Y_P3=32,
                    GV_CONV_Y2_P3=64, GV_CONV_MAXPOOL3S2=128, GV_CONV_MAXPOOL3S2_SAME=256, GV_CONV_POOL_ACT2=512)   # include/gvcnn_hip.h


def test_conv_flag_word():
    T = lambda vbuf=0, p3=False: SimpleNamespace(vbuf=vbuf, p3=p3)
    op = dict(x=T(), y=T(), y2=None, relu=True, split=0)
    assert L.conv_flags(op, False, F) == 1
    assert L.conv_flags(dict(op, relu=False, y2=T()), True, F) == 2
    assert L.conv_flags(dict(op, x=T(-1)), True, F) == 1 | 8 and L.conv_flags(dict(op, x=T(-1)), False, F) == 1
    assert L.conv_flags(dict(op, x=T(p3=True), y=T(p3=True), y2=T(p3=True), split=64), False, F) == 1 | 4 | 16 | 32 | 64
    assert L.conv_flags(dict(op, maxpool="VALID"), True, F) == 1 | 128
    assert L.conv_flags(dict(op, relu=False, x=T(-1), maxpool="SAME", pool_act=True), True, F) == 8 | 256 | 512 | 2
    with pytest.raises(AssertionError):
        L.conv_flags(dict(op, y2=T(p3=True)), False, F)


def test_fused_maxpool_predicate():
    ok = lambda **kw: L.fused_maxpool_ok(**dict(dict(cout=64, k=3, stride=1, oh=109, ow=109, pool_padding="VALID", x_c=32,
                                                     x_ld=32, x_is_input=False, x_p3=False, lowp=True, bf16x3=False), **kw))
    assert ok() and not ok(cout=96) and not ok(x_p3=True) and not ok(oh=2) and not ok(x_ld=36) and not ok(pool_padding="SAME")
    # fp32 storage: three-plane math only, and only where the 30-pixel strips beat the 16-pixel ones (Inception at 224 / 128)
    assert ok(lowp=False, bf16x3=True) and not ok(lowp=False) and not ok(lowp=False, bf16x3=True, oh=61, ow=61)
    stem = dict(x_is_input=True, x_c=3, x_ld=3, k=7, stride=2, oh=112, ow=112, pool_padding="SAME")
    assert ok(**stem) and not ok(**dict(stem, oh=49, ow=49)) and ok(**dict(stem, oh=49, ow=49, pool_padding="VALID"))
    assert not ok(**dict(stem, lowp=False, bf16x3=True)) and not ok(**dict(stem, stride=1))


# ---- tile choice ---------------------------------------------------------------------------------
def test_warm_repeat_rule():
    timed = [(0.30, 0), (0.10, 2), (0.12, 3), (0.11, 5), (0.20, 6)]          # tiles 1 and 4 were declined: absent
    assert L.warm_finalists(timed) == [2, 5, 3]
    assert L.warm_finalists(timed[:2]) == [2, 0] and L.warm_finalists([]) == []
    finals = [(0.105, 2), (0.101, 5), (0.13, 3)]                              # the second look moves tile 5 in front
    assert L.warm_order(timed, finals, 4) == (5, 0.101, [5, 2, 3, 6])
    assert L.warm_order(timed, finals, 9) == (5, 0.101, [5, 2, 3, 6, 0])
    assert L.warm_order(timed, finals, 1) == (5, 0.101, [5]) and L.warm_order(timed, finals, 0)[2] == [5]
    assert L.warm_order([], [], 4) == (0, float("inf"), [0])
    assert all(t not in L.warm_order(timed, finals, 9)[2] for t in (1, 4))


def test_in_sequence_rule():
    assert L.pick_in_sequence([5, 2, 3], {5: 0.2, 2: 0.1, 3: 0.3}) == 2
    assert L.pick_in_sequence([5, 2, 3], {5: 0.1, 2: 0.1, 3: 0.1}) == 5     # a tie keeps the warm-repeat winner
    assert L.pick_in_sequence([5, 2, 3], {5: 0.2, 2: 0.1, 3: 0.1}) == 2     # ... and the warm-repeat order behind it
    assert L.in_sequence_rounds(4, {3: [1]}) == 4 and L.in_sequence_rounds(2, {3: [1]}) == 2
    assert L.in_sequence_rounds(1, {3: [1]}) == 0 and L.in_sequence_rounds(0, {3: [1]}) == 0 and L.in_sequence_rounds(4, {}) == 0
