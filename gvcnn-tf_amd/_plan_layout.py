"""The pure arithmetic of the inference plan builder (backbones.BackbonePlan): arena placement, buffer assignment by
liveness, the cross-lane dependencies, the flag word of a convolution, the fusion form of every ResNet-v2 unit, the
fused conv -> max-pool predicate, the autotuner's selection rules.  Imports nothing from the package, so it loads (and
is tested) without the library.  Tensors are read through their attributes (vbuf, off, c, ld, p3) only."""


# ---- arenas ------------------------------------------------------------------------------------------
def place_filters(filters, w_elems, group):
    """Place the packed filters of ONE launch back to back in the weights arena (4-byte units) and round the group's end
    to 64 units, so that every launch's filter block stays 256-byte aligned.  group = [(name, kh, kw, cin, cout, packed
    size in units)]; appends (name, kh, kw, cin, cout, offset) to `filters`.  -> (offset of the first, new arena size)."""
    off = w_elems
    for name, kh, kw, cin, cout, n in group:
        filters.append((name, kh, kw, cin, cout, off))
        off += n
    return w_elems, (off + 63) // 64 * 64


def place_scale_shift(ss_specs, ss_elems, cols):
    """Place the (scale, shift) columns of ONE launch side by side in the scale/shift arena: a row of scales, then a row
    of shifts, each rounded to 4 channels.  cols = [(kind, name, c, eps, has_gamma)]; appends (kind, name, c, eps,
    has_gamma, scale offset, shift offset) to `ss_specs`.  -> (scale offset, shift offset, new arena size)."""
    cpad = (sum(c for _, _, c, _, _ in cols) + 3) // 4 * 4
    so, ho, cum = ss_elems, ss_elems + cpad, 0
    for kind, name, c, eps, has_gamma in cols:
        ss_specs.append((kind, name, c, eps, has_gamma, so + cum, ho + cum))
        cum += c
    return so, ho, ss_elems + 2 * cpad


# ---- buffers and lanes ------------------------------------------------------------------------------
def accesses(op):
    """What a launch touches: [(vbuf, is_write, first channel, end channel)] over x, res (reads), y, y2 (writes); the
    network input (vbuf < 0) is not a plan buffer."""
    acc = []
    for key, is_w in (("x", False), ("res", False), ("y", True), ("y2", True)):
        t = op.get(key)
        if t is not None and t.vbuf >= 0:
            lo = t.off % t.ld
            acc.append((t.vbuf, is_w, lo, lo + t.c))
    return acc


REUSE_DELAY = 16       # ops for which a buffer released by one lane is kept from the others (plans with lanes)


def assign_buffers(acc, lanes, vbufs, reuse_delay):
    """Physical buffers by liveness.  acc[i] = accesses of op i, lanes[i] its lane, vbufs[v] = (elements, kept, three-plane).
    A tensor gets its buffer at its first write and gives it back after its last access unless it is kept; a physical
    buffer holds either plain or three-plane tensors.  A buffer released by one lane is not handed to ANOTHER lane for
    `reuse_delay` ops: immediate reuse would order the independent branches behind each other (a write-after-read hazard
    the schedule then has to honour); memory is not the constraint.  The smallest free buffer that fits is taken; where
    none fits, the biggest reusable one is enlarged instead of adding one.
    -> (vmap {vbuf: physical}, physical sizes, physical formats)."""
    last_use, lanes_of = {}, {}
    for i, a in enumerate(acc):
        for v, _, _, _ in a:
            last_use[v] = i
            lanes_of.setdefault(v, set()).add(lanes[i])
    release = [[] for _ in acc]                    # in the order the tensors first appear
    for v, i in last_use.items():
        release[i].append(v)
    sizes, fmts, free, vmap = [], [], [], {}       # free: (physical, op index of the release, lanes that touched it)
    for i, a in enumerate(acc):
        for v, is_w, _, _ in a:
            if not is_w or v in vmap:
                continue
            need, fmt = vbufs[v][0], vbufs[v][2]
            ok = [f for f in free if (f[2] == {lanes[i]} or f[1] <= i - reuse_delay) and fmts[f[0]] == fmt]
            fit = [f for f in ok if sizes[f[0]] >= need]
            if fit:
                f = min(fit, key=lambda q: sizes[q[0]])
            elif ok:
                f = max(ok, key=lambda q: sizes[q[0]])
                sizes[f[0]] = need
            else:
                f = None
                sizes.append(need)
                fmts.append(fmt)
            if f is not None:
                free.remove(f)
            vmap[v] = len(sizes) - 1 if f is None else f[0]
        for v in release[i]:
            if v in vmap and not vbufs[v][1]:
                free.append((vmap[v], i, lanes_of[v]))
    return vmap, sizes, fmts


def lane_deps(acc, lanes, vmap):
    """Cross-lane dependencies: an op waits for every earlier op whose access to the same physical buffer conflicts with
    its own (read-after-write, write-after-read, write-after-write); accesses to disjoint channel slices of one tensor
    do not conflict.  What the op's own lane already implies is left out, and the latest conflicting op is taken first:
    it usually implies the older ones.  -> [sorted op indices] per op."""
    history = {}                      # physical -> [(op, is_write, vbuf, lo, hi)]
    hb = []                           # hb[i]: ops known complete before op i starts
    last_on_lane = {}
    out = []
    for i, a in enumerate(acc):
        need = set()
        for vb, is_w, lo, hi in a:
            for j, jw, jvb, jlo, jhi in history.get(vmap[vb], ()):
                if not (is_w or jw):
                    continue
                if jvb == vb and (hi <= jlo or jhi <= lo):
                    continue
                need.add(j)
        prev = last_on_lane.get(lanes[i])
        known = set() if prev is None else (hb[prev] | {prev})
        deps = []
        for j in sorted(need, reverse=True):
            if j in known:
                continue
            assert lanes[j] != lanes[i]
            deps.append(j)
            known |= hb[j] | {j}
        hb.append(known)
        last_on_lane[lanes[i]] = i
        for vb, is_w, lo, hi in a:
            history.setdefault(vmap[vb], []).append((i, is_w, vb, lo, hi))
        out.append(sorted(deps))
    return out


# ---- op records ----------------------------------------------------------------------------------
def conv_flags(op, lowp, F):
    """gv_conv_desc.flags of a plain convolution record.  lowp: 16-bit storage; F: where the GV_CONV_* constants live."""
    x, y, y2 = op["x"], op["y"], op["y2"]
    flags = F.GV_CONV_RELU if op["relu"] else 0
    if op["split"]:
        flags |= F.GV_CONV_SPLIT
    elif y2 is not None:
        flags |= F.GV_CONV_RELU2
    if lowp and x.vbuf < 0:
        flags |= F.GV_CONV_X_F32                    # the images stay fp32; the stem's loader rounds them
    if x.p3:
        flags |= F.GV_CONV_X_P3
    if y.p3:
        flags |= F.GV_CONV_Y_P3
    if y2 is not None and y2.p3:
        assert op["split"], "a three-plane second destination exists only for fused sibling convs"
        flags |= F.GV_CONV_Y2_P3
    if op.get("maxpool"):                           # y is the pooled tensor; oh / ow stay the convolution's
        flags |= F.GV_CONV_MAXPOOL3S2_SAME if op["maxpool"] == "SAME" else F.GV_CONV_MAXPOOL3S2
        if op.get("pool_act"):                      # ... stored through a second BatchNorm + ReLU
            flags |= F.GV_CONV_POOL_ACT2 | F.GV_CONV_RELU2
    return flags


def fused_maxpool_ok(cout, k, stride, oh, ow, pool_padding, x_c, x_ld, x_is_input, x_p3, lowp, bf16x3):
    """The classes GV_CONV_MAXPOOL3S2 / _SAME serve (include/gvcnn_hip.h) for a k x k / stride convolution with an
    oh x ow map.  16-bit storage: 3x3 / stride 1 from 32 to 64 channels (VALID pool), or a 3x3 / 7x7 stride-2 stem on the
    fp32 images at 64 channels (VALID, or SAME on an even map); fp32 storage under three-plane math: the halo kernel's
    30-pixel strip form, VALID pool, where it beats the 16-pixel one."""
    if cout != 64 or x_p3 or min(oh, ow) < 3:
        return False
    if not lowp:
        return (bf16x3 and pool_padding == "VALID" and k == 3 and stride == 1 and x_c == 32 and not x_is_input
                and x_ld % 4 == 0 and -(-ow // 16) * 16 * 5 > -(-ow // 30) * 32 * 4)
    if pool_padding == "SAME" and (oh % 2 or ow % 2):
        return False
    if x_is_input:                                  # the network input: the stem strip kernel
        return k in (3, 7) and stride == 2 and x_c == 3
    return pool_padding == "VALID" and k == 3 and stride == 1 and x_c == 32 and x_ld % 8 == 0


def chain_ok(c, ld, p3, lowp):
    """May a conv3 over c channels (-> 4c) and the next unit's preact + conv1 be one launch (csrc/conv_chain.hip)?"""
    return lowp and c in (64, 128) and ld % 8 == 0 and not p3


# ---- ResNet-v2 unit forms ------------------------------------------------------------------------
def resnet_unit_forms(units, lowp, proj0, fuse_chain, fuse_unit, fuse_pair, defer_preact):
    """How every bottleneck unit of a ResNet-v2 is emitted.  units = [(block, base depth, unit index, units of the block,
    stride)]; proj0: the first unit's pre-activation was written beside where its conv2 writes (GV_CHAIN_PROJ's input).
    -> [(shortcut, tail)] with
    shortcut  "in_gemm"     a projection inside conv3's GEMM (no tensor, no launch)
              "identity"    the unit's input            "subsampled"  ... through a 1x1 / stride max pool
              "pair"        a projection in ONE GEMM with conv1      "conv"  a projection launch of its own
    tail      "unit"        conv2 + conv3 + the next unit's preact + conv1 as one launch
              "chain"       conv3 + the next preact + conv1         "chain_proj"  ... with the in_gemm shortcut
              "deferred"    conv3 writes the sum; the next conv1's loader applies the preact
              "stored"      conv3 writes the sum and the next preact    "last"  no next unit.
    After a unit / chain / chain_proj tail the next unit's conv1 exists already."""
    forms, depth_in, deferred, c1_ready = [], 64, False, False
    for i, (_, base, _, _, stride) in enumerate(units):
        depth = base * 4
        nbase = units[i + 1][1] if i + 1 < len(units) else None
        proj = i == 0 and proj0 and stride == 1 and depth != depth_in and depth_in == base and nbase is not None and \
            nbase * 4 == depth
        if proj:
            shortcut = "in_gemm"
        elif depth == depth_in:
            shortcut = "identity" if stride == 1 else "subsampled"
        elif stride == 1 and fuse_pair and not deferred and base % 8 == 0 and not c1_ready and base >= 128:
            # (block1's pair — 64 + 256 columns over K = 64 — measured slower than its two launches: 0.283 against 0.269 ms)
            shortcut = "pair"
        else:
            shortcut = "conv"
        # the next unit keeps this depth (identity shortcut, conv1 the pre-activation's only reader) and the bottleneck
        # depth is one the chain kernel serves
        chains = nbase is not None and nbase * 4 == depth and bool(fuse_chain) and chain_ok(base, base, False, lowp)
        assert chains or not proj
        # whole units where that pays: d = 64.  At d = 128 the unit launch measured level with chain + conv2 (0.276 against
        # 0.166 + 0.107 ms): its conv2 phase is matrix-heavy and its one 8-wave workgroup per CU runs the phases in
        # lockstep; fuse_unit="all" asks for it anyway.  (stride 1: the strided unit is a block's last)
        if nbase is None:
            tail = "last"
        elif chains:
            whole = bool(fuse_unit) and stride == 1 and (base <= 64 or fuse_unit == "all") and not proj
            tail = "unit" if whole else "chain_proj" if proj else "chain"
        elif defer_preact and nbase * 4 == depth and depth <= 1024:
            # not in block4 (2048 channels over 7x7 maps): its conv3 is no longer HBM-bound and the conv1 loses more on
            # the register-staged loader than the conv3 gains
            tail = "deferred"
        else:
            tail = "stored"
        forms.append((shortcut, tail))
        depth_in, deferred, c1_ready = depth, tail == "deferred", tail in ("unit", "chain", "chain_proj")
    return forms


# ---- autotune ------------------------------------------------------------------------------------
def warm_finalists(timed):
    """Pass 1, first look: timed = [(ms, tile)] of the tiles that ran (declined ones are absent).  The three fastest get
    a second, longer look: one noisy sample must not pick the tile of a 0.1 ms launch."""
    return [t for _, t in sorted(timed)[:3]]


def warm_order(timed, finals, in_sequence):
    """Pass 1, choice: finals = [(ms, tile)] of the finalists' second look.  -> (best tile, its ms, the candidates of
    pass 2: the winner, then the others by their first look, `in_sequence` of them at most and one at least);
    (0, inf, [0]) where no tile ran."""
    best_ms, best = min(finals) if finals else (float("inf"), 0)
    order = [best] + [t for _, t in sorted(timed) if t != best]
    return best, best_ms, order[:max(int(in_sequence), 1)]


def in_sequence_rounds(in_sequence, cands):
    """Rounds of pass 2; 0: pass 1 only."""
    return int(in_sequence) if int(in_sequence) > 1 and cands else 0


def pick_in_sequence(cands, seq_ms):
    """Pass 2: the candidate that was fastest where it actually runs; a tie keeps the warm-repeat order."""
    return min(cands, key=lambda t: (seq_ms[t], cands.index(t)))
