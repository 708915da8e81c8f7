"""Images and reference restatements for the PNG encoder tests (not a test file): the image matrix, a numpy
restatement of the five line filters and of the adaptive rule (the reference for the filtered bytes; zlib.decompress is
the reference for the stream), ctypes wrappers around the two entry points, and the dump that
tests/native/png_enc_core_check.cpp reads."""
import os
import struct
import zlib

import numpy as np

ADAPTIVE, AUTO, RGB = 5, 0, 1
FILTERS = (ADAPTIVE, 0, 1, 2, 3, 4)
COLORS = (AUTO, RGB)


def lib():
    from gvcnn_tf_amd import _lib
    return _lib.load()


def seg_bytes():
    return int(lib().gv_png_encode_segment_bytes())


# ---- content --------------------------------------------------------------------------------------------------------
def _gray(g):
    g = np.ascontiguousarray(g, np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], axis=2))


def constant(w, h, v=77):
    return _gray(np.full((h, w), v, np.uint8))


def ramp(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return _gray((yy * 3 + xx) % 256)


def gray_noise(w, h, seed):
    return _gray(np.random.RandomState(seed).randint(0, 256, size=(h, w)))


def rgb_noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def one_pixel(w, h, where):
    """gray everywhere but one pixel with G != R: the first or the last"""
    img = ramp(w, h)
    y, x = (0, 0) if where == "first" else (h - 1, w - 1)
    img[y, x, 1] ^= 0x40
    return img


def disc(w, h):
    """a shaded disc on white, like a rendered view"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 0.4 * min(w, h) + 0.5
    d = np.sqrt((yy - (h - 1) / 2) ** 2 + (xx - (w - 1) / 2) ** 2)
    return _gray(np.where(d < r, 60 + 150 * np.clip(1 - d / r, 0, 1), 255))


def runs_row(lengths):
    """a one-row gray image whose bytes are runs of exactly these lengths between distinct bytes"""
    out = [199]
    for k, n in enumerate(lengths):                              # values 10 + k, separators 200 + k: all distinct
        out += [10 + k] * n + [200 + k]
    return _gray(np.array(out, np.uint8)[None, :])


def run_free(w, h, seed):
    """gray, no byte equal to its left neighbour (and none equal to the filter byte 0 of its row): values 1 + a
    two-sided geometric variable over 64 values with ratio 0.8, centred, redrawn where two neighbours agree"""
    rng = np.random.RandomState(seed)
    k = np.arange(64)
    p = 0.8 ** np.abs(k - 32)
    p /= p.sum()
    g = rng.choice(64, size=(h, w), p=p) + 1
    for y in range(h):
        for x in range(w):
            left = g[y, x - 1] if x else 0
            while g[y, x] == left:
                g[y, x] = rng.choice(64, p=p) + 1
    return _gray(g)


RUN_EDGES = (2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518)
# the smallest match length of each of the 29 length symbols 257..285 (RFC 1951, 3.2.5)
LENGTH_BASES = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_IMAGES = None


def images():
    """[(name, uint8 [h, w, 3])] — built once, shared, never modified"""
    global _IMAGES
    if _IMAGES is not None:
        return _IMAGES
    SEG = seg_bytes()
    out = []
    for w, h in ((1, 1), (7, 1), (1, 7), (5, 9), (17, 9), (64, 9)):  # raw streams far shorter than a segment
        s = "%dx%d" % (w, h)
        out += [(s + "-constant", constant(w, h)), (s + "-ramp", ramp(w, h)), (s + "-gray-noise", gray_noise(w, h, w + h)),
                (s + "-rgb-noise", rgb_noise(w, h, w * h)), (s + "-first-pixel", one_pixel(w, h, "first")),
                (s + "-last-pixel", one_pixel(w, h, "last")), (s + "-disc", disc(w, h))]
    we = SEG // 64 - 1                                           # gray: 64 rows of 1 + we bytes are exactly one segment
    out += [("exact-seg-gray-ramp", ramp(we, 64)), ("exact-seg-gray-noise", gray_noise(we, 64, 5))]
    assert 64 * (1 + we) == SEG and SEG % 16 == 0
    out.append(("exact-seg-rgb-noise", rgb_noise(5, SEG // 16, 6)))          # RGB: rows of 16 bytes
    out += [("100x100-disc", disc(100, 100)), ("100x100-gray-noise", gray_noise(100, 100, 7)),      # a boundary mid-row
            ("100x100-last-pixel", one_pixel(100, 100, "last")), ("100x100-constant", constant(100, 100, 200))]
    assert SEG % 101 and SEG % 301
    out += [("224-disc", disc(224, 224)), ("224-constant", constant(224, 224, 0)), ("224-rgb-noise", rgb_noise(224, 224, 8))]
    out += [("299-disc", disc(299, 299)), ("299-first-pixel", one_pixel(299, 299, "first"))]
    out.append(("runs", runs_row(RUN_EDGES)))
    # every literal and one run per length symbol: all 286 symbols of the literal / length alphabet in one segment
    every = np.concatenate([np.random.RandomState(10).permutation(256), runs_row([n + 1 for n in LENGTH_BASES])[0, :, 0]])
    assert every.size + 1 <= SEG
    out.append(("all-286-symbols", _gray(every[None, :].astype(np.uint8))))
    g = np.random.RandomState(9).randint(0, 256, size=SEG + 600)
    g[SEG - 150:SEG + 150] = 33                                  # a run of 300 across the first boundary
    out.append(("run-across-boundary", _gray(g[None, :].astype(np.uint8))))
    _IMAGES = out
    return out


# ---- the reference: filters in numpy --------------------------------------------------------------------------------
def filter_candidates(rows, bpp):
    """uint8 [h, rowbytes] -> uint8 [5, h, rowbytes]: every row under every filter type (PNG specification 9.2, Paeth's
    tie order a, b, c)"""
    x = rows.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([((x - p) & 255).astype(np.uint8) for p in (0 * x, a, b, (a + b) >> 1, paeth)])


def filter_costs(cand):
    """[5, h, rowbytes] -> int64 [5, h]: sum of |signed residual|"""
    v = cand.astype(np.int64)
    return np.where(v < 128, v, 256 - v).sum(axis=2)


def expected_raw(img, filt, color):
    """(colour type, filter types [h], the raw stream as uint8 [h, 1 + w * ch]) the encoder must produce"""
    h, w, _ = img.shape
    gray = color == AUTO and np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 1], img[..., 2])
    ch = 1 if gray else 3
    rows = np.ascontiguousarray(img[..., :ch]).reshape(h, w * ch)
    cand = filter_candidates(rows, ch)
    if filt == ADAPTIVE:
        types = np.argmin(filter_costs(cand), axis=0)            # (argmin: the first, i.e. the lowest type on a tie)
    else:
        types = np.full(h, filt)
    raw = np.empty((h, 1 + w * ch), np.uint8)
    raw[:, 0] = types
    raw[:, 1:] = cand[types, np.arange(h)]
    return (0 if gray else 2), types, raw


# ---- the entry points -------------------------------------------------------------------------------------------------
def encode_host(views, filt=ADAPTIVE, color=AUTO, fill=0xA5):
    """uint8 [n, h, w, 3] -> (rc, out uint8 [n, bound] pre-filled with `fill`, length [n], colour type [n])"""
    L = lib()
    views = np.ascontiguousarray(views, np.uint8)
    n, h, w, _ = views.shape
    stride = int(L.gv_png_encode_bound(h, w))
    out = np.full((n, stride), fill, np.uint8)
    length, ctype = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    rc = L.gv_png_encode_host(views.ctypes.data, n, h, w, filt, color, out.ctypes.data, stride, length.ctypes.data,
                              ctype.ctypes.data)
    return rc, out, length, ctype


def stream(img, filt=ADAPTIVE, color=AUTO):
    """one image -> (zlib stream bytes, colour type) through the host twin"""
    rc, out, length, ctype = encode_host(img[None], filt, color)
    assert rc == 0
    assert (out[0, length[0]:] == 0xA5).all(), "written past length"
    return out[0, :length[0]].tobytes(), int(ctype[0])


def mixed_batch(n=70, w=21, h=13):
    """n views of one size, content mixed"""
    makers = (lambda i: constant(w, h, i), lambda i: ramp(w, h), lambda i: gray_noise(w, h, i), lambda i: rgb_noise(w, h, i),
              lambda i: one_pixel(w, h, "first"), lambda i: one_pixel(w, h, "last"), lambda i: disc(w, h))
    return np.stack([makers[i % len(makers)](i) for i in range(n)])


# ---- the dump tests/native/png_enc_core_check.cpp reads -----------------------------------------------------------
def dump(path):
    """records of six int32 (w, h, filter, colour constant, expected colour type, raw bytes), the pixels [h, w, 3], the
    expected raw stream"""
    with open(path, "wb") as f:
        for name, img in images():
            for filt in FILTERS:
                for color in COLORS:
                    if max(img.shape) > 200 and (filt, color) not in ((ADAPTIVE, AUTO), (4, RGB), (0, AUTO)):
                        continue
                    ctype, _, raw = expected_raw(img, filt, color)
                    f.write(struct.pack("<6i", img.shape[1], img.shape[0], filt, color, ctype, raw.size))
                    f.write(img.tobytes() + raw.tobytes())


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump(sys.argv[1])
