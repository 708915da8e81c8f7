"""The pure arithmetic of the training engine (training.TrainGVCNN): parity-class geometry of stride-2 data gradients,
the flat parameter layout, the autotuner's selection rule.  Imports nothing from the package, so it loads (and is
tested) without the library."""


def s2_parity_classes(kh, kw, pad_t, pad_l, ih, iw):
    """The data gradient of a stride-2 convolution (kh x kw, padding (pad_t, pad_l), input ih x iw) as FOUR parity
    classes (gv_conv_desc.y_step): dX at rows of parity py / columns of parity px only receives the taps
    r = (py + pad) mod 2, +2, ... — a small stride-1 convolution over the un-dilated dZ per class, 1/4 of the
    multiply-adds of the zero-dilated form.  -> four dicts (r0, s0: first tap; th, tw: taps per class; pad_t, pad_l:
    zero rows / columns in front of dZ; A, B: class outputs), or None where a class has no tap or no pixel."""
    cls = []
    for py in (0, 1):
        for px in (0, 1):
            r0, s0 = (py + pad_t) % 2, (px + pad_l) % 2
            th, tw = len(range(r0, kh, 2)), len(range(s0, kw, 2))
            pt = (th - 1) - (py + pad_t - r0) // 2
            pl = (tw - 1) - (px + pad_l - s0) // 2
            A, B = len(range(py, ih, 2)), len(range(px, iw, 2))
            if th < 1 or tw < 1 or pt < 0 or pl < 0 or A < 1 or B < 1:
                return None
            cls.append(dict(py=py, px=px, r0=r0, s0=s0, th=th, tw=tw, pad_t=pt, pad_l=pl, A=A, B=B))
    return cls


def flat_layout(train_names, numels, fused_of):
    """Offsets of the trainable variables in the flat fp32 buffers: the conv filters ("/weights") first, the rest behind
    them, every slot rounded up to 16 elements.  fused_of {member name: (block key, block elements)}: the members of a
    fused sibling GEMM share ONE slot, at the position of the block's first member.
    -> (offs {name: offset} of the other variables, {block key: offset}, n_wd = first offset of a non-filter variable
    (total where there is none), total)."""
    order = [k for k in train_names if k.endswith("/weights")] + [k for k in train_names if not k.endswith("/weights")]
    offs, block_off, n_wd, total = {}, {}, None, 0
    for k in order:
        if n_wd is None and not k.endswith("/weights"):
            n_wd = total
        if k in fused_of:
            key, n = fused_of[k]
            if key not in block_off:
                block_off[key] = total
                total += (n + 15) // 16 * 16
            continue
        offs[k] = total
        total += (numels[k] + 15) // 16 * 16
    return offs, block_off, total if n_wd is None else n_wd, total


def pick_tile(candidates, folding_only=False):
    """The autotuner's choice among measured rows (tile index, ms or None = the launch was declined, folded = the
    launch that also produces the BatchNorm sums; a fusable layer's plain row carries its separate sums passes in ms).
    Visited in increasing tile index, a tile's folded row before its plain one; a row replaces the incumbent only when
    strictly faster.  folding_only: plain rows do not compete (the parity classes of a layer fold all, or none).
    -> (best, best_ms, best_fused); (0, inf, False) without a valid row."""
    best, best_ms, best_fused = 0, float("inf"), False
    for tile, ms, folded in sorted(candidates, key=lambda r: (r[0], not r[2])):
        if ms is None or (folding_only and not folded):
            continue
        if ms < best_ms:
            best, best_ms, best_fused = tile, ms, bool(folded)
    return best, best_ms, best_fused
