"""The pure arithmetic of the training engine (gvcnn-tf_amd/_train_layout.py): parity classes of a stride-2 data
gradient against the transposed convolution written out tap by tap, the flat parameter layout, the autotuner's
selection rule.  The module is loaded from its file: no device, no library."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gv_train_layout", os.path.join(ROOT, "gvcnn-tf_amd", "_train_layout.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)


def _taps_1d(k, pad, n_in, y):
    """The transposed convolution along one axis, by its definition: {forward tap r: dZ index o} over every pair with
    2*o + r - pad == y.  o runs past both ends of dZ: those positions are zeros for the forward convolution's output
    size whatever it is, and the class must place its taps on the same ones."""
    return {r: o for r in range(k) for o in range(-k, n_in + k) if 2 * o + r - pad == y}


def _class_taps_1d(r0, t, pad, a):
    """What one class computes along one axis for its output a: a stride-1 convolution with t taps over dZ padded by
    `pad` in front, whose tap j holds forward tap r0 + 2*(t-1-j) (the flipped filter of a data gradient):
    {forward tap: dZ index}."""
    return {r0 + 2 * (t - 1 - j): a + j - pad for j in range(t)}


S2_CASES = [
    (3, 3, 0, 0, 9, 9), (3, 3, 0, 0, 10, 10),      # Inception's VALID stride-2 layers: an odd and an even map
    (3, 3, 1, 1, 8, 8),                            # ResNet's explicitly padded conv2
    (7, 7, 2, 2, 16, 16), (7, 7, 3, 3, 16, 16),    # ResNet conv1 under SAME
    (2, 7, 0, 3, 12, 12), (3, 7, 1, 3, 12, 11),    # one tap per row class; 1 and 2
]


@pytest.mark.parametrize("kh,kw,pad_t,pad_l,ih,iw", S2_CASES)
def test_s2_parity_classes_enumerate_the_transposed_convolution(kh, kw, pad_t, pad_l, ih, iw):
    cls = L.s2_parity_classes(kh, kw, pad_t, pad_l, ih, iw)
    assert cls is not None and [(c["py"], c["px"]) for c in cls] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for c in cls:
        rows, cols = range(c["py"], ih, 2), range(c["px"], iw, 2)
        assert (c["A"], c["B"]) == (len(rows), len(cols))
        # every dX pixel of this parity: the class's taps and the dZ pixels they read ARE the transposed convolution's
        # (dZ indices outside the map are the zero padding on either side: they must agree too)
        for axis, (k, pad, n, r0, t, cpad, pix) in enumerate(((kh, pad_t, ih, c["r0"], c["th"], c["pad_t"], rows),
                                                              (kw, pad_l, iw, c["s0"], c["tw"], c["pad_l"], cols))):
            assert list(range(r0, k, 2)) == sorted(_class_taps_1d(r0, t, cpad, 0)), axis
            for a, y in enumerate(pix):
                assert _class_taps_1d(r0, t, cpad, a) == _taps_1d(k, pad, n, y), (axis, y)


def test_s2_parity_classes_decline_a_class_without_tap_or_pixel():
    # one tap along an axis reaches only one parity of it: the other class has nothing to compute
    assert _taps_1d(1, 0, 8, 1) == {} and _taps_1d(1, 0, 8, 0) == {0: 0}
    assert L.s2_parity_classes(1, 1, 0, 0, 8, 8) is None
    assert L.s2_parity_classes(1, 7, 0, 3, 12, 12) is None      # (1x7 with padding (0, 3): no tap on the odd rows)
    assert L.s2_parity_classes(7, 1, 3, 0, 12, 12) is None
    assert L.s2_parity_classes(3, 3, 1, 1, 1, 8) is None        # a 1-row map has no odd row
    assert L.s2_parity_classes(3, 3, 1, 1, 8, 1) is None


def _layout_case():
    names = ["a/weights", "blk/b0/weights", "a/BatchNorm/beta", "mid/weights", "blk/b2/weights", "a/BatchNorm/gamma",
             "blk/b1/weights", "Logits/weights", "Logits/biases"]
    numels = {"a/weights": 3 * 3 * 3 * 5, "mid/weights": 100, "a/BatchNorm/beta": 5, "a/BatchNorm/gamma": 5,
              "Logits/weights": 7 * 40, "Logits/biases": 40, "blk/b0/weights": 24 * 8, "blk/b1/weights": 24 * 3,
              "blk/b2/weights": 24 * 6}
    cin, couts = 24, (8, 3, 6)
    fused_of = {"blk/b%d/weights" % i: ("blk", cin * sum(couts)) for i in range(3)}
    return names, numels, fused_of, cin * sum(couts)


def test_flat_layout():
    names, numels, fused_of, block = _layout_case()
    c16 = lambda n: (n + 15) // 16 * 16
    offs, block_off, n_wd, total = L.flat_layout(names, numels, fused_of)
    assert set(offs) == set(names) - set(fused_of) and set(block_off) == {"blk"}
    slots = sorted([(o, c16(numels[k]), k) for k, o in offs.items()] + [(block_off["blk"], c16(block), "blk")])
    assert all(o % 16 == 0 for o, _, _ in slots)
    assert slots[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(slots, slots[1:]))     # dense, no overlap
    assert slots[-1][0] + slots[-1][1] == total
    # filters first, in the order given; the block ONCE, where its first member stands
    assert [k for _, _, k in slots] == ["a/weights", "blk", "mid/weights", "Logits/weights", "a/BatchNorm/beta",
                                        "a/BatchNorm/gamma", "Logits/biases"]
    assert block % 16 and block_off["blk"] == c16(numels["a/weights"])
    assert n_wd == offs["a/BatchNorm/beta"] == min(o for k, o in offs.items() if not k.endswith("/weights"))
    # nothing but filters: the L2 region is the whole buffer
    only_w = [k for k in names if k.endswith("/weights")]
    offs, block_off, n_wd, total = L.flat_layout(only_w, numels, fused_of)
    assert n_wd == total == sum(c16(numels[k]) for k in only_w if k not in fused_of) + c16(block)


def test_pick_tile():
    inf = float("inf")
    assert L.pick_tile([]) == (0, inf, False)
    assert L.pick_tile([(1, None, True), (1, None, False), (2, None, False)]) == (0, inf, False)
    # a tie keeps the lower index (strict <), whatever order the rows come in
    assert L.pick_tile([(1, 0.5, False), (2, 0.5, False), (3, 0.5, False)]) == (1, 0.5, False)
    assert L.pick_tile([(3, 0.5, False), (2, 0.5, False), (2, 0.7, True)]) == (2, 0.5, False)
    # ... and inside one tile the folded launch, which is visited first
    assert L.pick_tile([(4, 0.25, False), (4, 0.25, True)]) == (4, 0.25, True)
    # folded against plain + the separate sums passes (0.08): either can win
    extra = 0.08
    assert L.pick_tile([(1, 0.20, True), (1, 0.15 + extra, False)]) == (1, 0.20, True)
    assert L.pick_tile([(1, 0.27, True), (1, 0.12 + extra, False)]) == (1, 0.12 + extra, False)
    assert L.pick_tile([(1, None, True), (1, 0.3, False), (2, 0.25, True)]) == (2, 0.25, True)
    # parity classes of a layer that folds the sums: plain rows do not compete
    rows = [(1, 0.1, False), (2, 0.4, True), (3, 0.3, True), (4, 0.05, False)]
    assert L.pick_tile(rows, folding_only=True) == (3, 0.3, True)
    assert L.pick_tile(rows) == (4, 0.05, False)
    assert L.pick_tile([(1, 0.1, False)], folding_only=True) == (0, inf, False)
