"""PNG files and zlib streams for the decoder tests (not a test file): a numpy / zlib PNG writer that controls what a
decoder can meet — the filter type of every row, how the stream is deflated, where it is cut into IDAT chunks, the colour
type and the palette — plus hand-assembled DEFLATE streams (a bit writer with the fixed code) for what zlib never
emits: a match at distance 32 768 and every malformed stream.  Expected pixels always come from the array a file was
written from (and the tests compare records.decode_png with it too)."""
import os
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
(OK, TRUNCATED, BAD_HEADER, BAD_BLOCK, BAD_CODES, BAD_DISTANCE, TOO_LONG, TOO_SHORT, BAD_CHECKSUM, BAD_FILTER,
 BAD_PALETTE_INDEX) = range(11)


# ---- filters ------------------------------------------------------------------------------------------------------
def _filtered(cur, prev, bpp, ft):
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
    c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
    if ft == 0:
        p = np.zeros_like(cur)
    elif ft == 1:
        p = a
    elif ft == 2:
        p = prev
    elif ft == 3:
        p = (a + prev) >> 1
    else:
        pa, pb, pc = np.abs(prev - c), np.abs(a - c), np.abs(a + prev - 2 * c)
        p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
    return ((cur - p) & 255).astype(np.uint8)


def filter_rows(arr, filters=0):
    """uint8 [h, w, ch] -> the bytes a PNG deflates.  filters: one type for every row, a list (row y gets
    filters[y % len]), ("seed", k) for one drawn per row, or "adaptive" (the smallest sum of absolute residuals)."""
    h, w, ch = arr.shape
    rows = arr.reshape(h, w * ch)
    if isinstance(filters, tuple) and filters[0] == "seed":
        filters = list(np.random.RandomState(filters[1]).randint(0, 5, size=h))
    out = bytearray()
    for y in range(h):
        prev = rows[y - 1] if y else np.zeros(w * ch, np.uint8)
        if isinstance(filters, str):
            cand = [_filtered(rows[y], prev, ch, ft) for ft in range(5)]
            ft = int(np.argmin([np.abs(c.astype(np.int8).astype(np.int32)).sum() for c in cand]))
            line = cand[ft]
        else:
            ft = int(filters if np.isscalar(filters) else filters[y % len(filters)])
            line = _filtered(rows[y], prev, ch, ft)
        out += bytes([ft]) + line.tobytes()
    return bytes(out)


# ---- deflate variants ---------------------------------------------------------------------------------------------
DEFLATE = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "huffman": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
    "filtered": dict(level=6, strategy=zlib.Z_FILTERED),
    "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9),
    "w9": dict(level=6, wbits=9), "w10": dict(level=6, wbits=10), "w11": dict(level=6, wbits=11),
    "w12": dict(level=6, wbits=12), "w13": dict(level=6, wbits=13), "w14": dict(level=6, wbits=14),
    "w15": dict(level=6, wbits=15),
    "flush": dict(level=6, flush=True),
}


def deflate(raw, how="l6"):
    kw = dict(DEFLATE[how])
    flush = kw.pop("flush", False)
    co = zlib.compressobj(kw.pop("level"), zlib.DEFLATED, kw.pop("wbits", 15), 9, kw.pop("strategy", zlib.Z_DEFAULT_STRATEGY))
    if not flush:
        return co.compress(raw) + co.flush()
    # a full flush in mid-stream: an empty stored block, and the next block starts off a byte boundary's far side
    cut = max(1, len(raw) // 3)
    return co.compress(raw[:cut]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[cut:]) + co.flush()


# ---- the file -----------------------------------------------------------------------------------------------------
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def wrap_png(w, h, ctype, zbytes, palette=None, splits=()):
    """PNG around a ready zlib stream, cut into IDAT chunks at the byte positions `splits`."""
    out = SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
    if palette is not None:
        out += _chunk(b"PLTE", np.ascontiguousarray(palette, np.uint8).tobytes())
    cuts = [0] + sorted(int(s) % (len(zbytes) + 1) for s in splits) + [len(zbytes)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += _chunk(b"IDAT", zbytes[a:b])
    return out + _chunk(b"IEND", b"")


def write_png(arr, ctype, palette=None, filters=0, how="l6", splits=()):
    arr = np.ascontiguousarray(arr, np.uint8)
    h, w, ch = arr.shape
    assert ch == CHANNELS[ctype]
    return wrap_png(w, h, ctype, deflate(filter_rows(arr, filters), how), palette, splits)


def expected(arr, ctype, palette=None):
    """What tf.image.decode_png(channels=3) makes of the array a file was written from."""
    arr = np.asarray(arr, np.uint8)
    if ctype == 3:
        return np.asarray(palette, np.uint8)[arr[..., 0]]
    if ctype in (0, 4):
        return np.repeat(arr[..., :1], 3, axis=2)
    return np.ascontiguousarray(arr[..., :3])


# ---- DEFLATE by hand: the fixed code ------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):                                 # least significant bit first (header fields, extra bits)
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                                 # a Huffman code: most significant bit first
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def lit(self, s):                                            # literal / length symbol of the fixed code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):
        if length == 258:
            self.lit(285)
        else:
            for s in range(257, 285):
                eb = 0 if s < 265 else (s - 261) >> 2
                base = s - 254 if s < 265 else 3 + ((4 + ((s - 261) & 3)) << eb)
                if base <= length < base + (1 << eb):
                    self.lit(s)
                    self.put(length - base, eb)
                    break
        for s in range(30):
            eb = 0 if s < 4 else (s >> 1) - 1
            base = s + 1 if s < 4 else 1 + ((2 + (s & 1)) << eb)
            if base <= dist < base + (1 << eb):
                self.code(s, 5)
                self.put(dist - base, eb)
                return
        raise ValueError(dist)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


def zwrap(body, data):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)


def far_match_case():
    """128 x 129 RGBA whose 66 177 filtered bytes are 32 768 random bytes followed by copies of them, deflated by hand as
    32 768 literals and then matches of length 258 at distance 32 768 (zlib itself stops at 32 506)."""
    w, h, rb = 128, 129, 128 * 4 + 1
    total = h * rb
    r = np.random.RandomState(11).randint(0, 256, size=32768).astype(np.uint8)
    for k in range(h):                                           # the filter bytes (type 0) must recur with the period
        r[(k * rb) % 32768] = 0
    raw = np.tile(r, 3)[:total]
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    for v in r:
        b.lit(int(v))
    left = total - 32768
    while left:
        n = min(258, left)
        if 0 < left - n < 3:                                     # (a match is at least 3 bytes long)
            n -= 3
        b.match(n, 32768)
        left -= n
    b.lit(256)
    arr = raw.reshape(h, rb)[:, 1:].reshape(h, w, 4)
    return wrap_png(w, h, 6, zwrap(b.bytes(), raw.tobytes())), expected(arr, 6)


# ---- the case matrix ----------------------------------------------------------------------------------------------
def blob(size, seed=0):
    """A gray shaded blob on white, like tools/pipeline_bench.py's render."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    img = np.full((size, size), 255.0, np.float32)
    for _ in range(4):
        (cx, cy), r = rng.uniform(0.25, 0.75, 2) * size, rng.uniform(0.1, 0.3) * size
        d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
        shade = 60 + 150 * np.clip(1 - d / r, 0, 1) + rng.uniform(-3, 3, size=d.shape)
        img = np.where(d < r, shade, img)
    g = np.clip(img, 0, 255).astype(np.uint8)
    return np.stack([g, g, g], axis=2)


def _img(rng, w, h, ch):
    """Smooth + noisy content: every deflate variant finds matches AND literals in it."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((yy * 5 + xx * 3) % 256).astype(np.uint8)
    planes = [base, base[::-1], rng.randint(0, 256, size=base.shape).astype(np.uint8), (base // 2 + 100).astype(np.uint8)]
    return np.stack(planes[:ch], axis=2)


_CASES = None


def cases():
    """[(name, png bytes, expected uint8 [h, w, 3])] — built once, shared, never modified."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.RandomState(7)
    out = []

    def add(name, arr, ctype, palette=None, **kw):
        out.append((name, write_png(arr, ctype, palette, **kw), expected(arr, ctype, palette)))
    # sizes
    add("1x1-gray", _img(rng, 1, 1, 1), 0)
    add("3x5-rgb", _img(rng, 3, 5, 3), 2, filters=("seed", 1))
    add("17x31-graya", _img(rng, 17, 31, 2), 4, filters=("seed", 2))
    add("65x2-rgba", _img(rng, 65, 2, 4), 6, filters=[4, 3])
    add("150x150-rgb-stored", _img(rng, 150, 150, 3), 2, how="stored")
    out.append(("128x129-rgba-dist32768",) + far_match_case())
    add("constant", np.full((40, 50, 3), 77, np.uint8), 2)
    add("224-blob-adaptive", blob(224), 2, filters="adaptive")
    add("1100x2-rgb-two-segments", _img(rng, 1100, 2, 3), 2, filters=[1, 4])     # a row longer than one LDS segment
    add("800x3-rgba-two-segments", _img(rng, 800, 3, 4), 6, filters=[3, 4, 2])
    # each filter forced, and mixed runs, on every colour type
    pal256 = rng.randint(0, 256, size=(256, 3)).astype(np.uint8)
    for ctype in (0, 2, 3, 4, 6):
        arr = _img(rng, 19, 13, CHANNELS[ctype])
        for ft in (0, 1, 2, 3, 4, ("seed", 3 + ctype)):
            add("c%d-f%s" % (ctype, ft if isinstance(ft, int) else "mix"), arr, ctype, pal256 if ctype == 3 else None, filters=ft)
    # palettes of 1, 2 and 256 entries
    add("pal1", np.zeros((5, 7, 1), np.uint8), 3, np.array([[9, 8, 7]], np.uint8))
    add("pal2", rng.randint(0, 2, size=(9, 11, 1)).astype(np.uint8), 3, np.array([[1, 2, 3], [250, 251, 252]], np.uint8), filters=1)
    add("pal256", rng.randint(0, 256, size=(16, 16, 1)).astype(np.uint8), 3, pal256, filters=("seed", 9))
    # every deflate variant (40 x 30: more than 512 bytes, so the smallest window is exceeded)
    arr = _img(rng, 40, 30, 3)
    for how in DEFLATE:
        add("deflate-" + how, arr, 2, filters=("seed", 4), how=how)
    # IDAT splits: inside the 2-byte header, inside the trailer, many small chunks
    z = len(deflate(filter_rows(arr, 1), "l6"))
    for name, splits in (("hdr", (1,)), ("trailer", (z - 2,)), ("many", tuple(range(1, z, 37))), ("empty", (5, 5))):
        add("split-" + name, arr, 2, filters=1, splits=splits)
    _CASES = out
    return out


def pillow_cases():
    """Pillow-written files of every mode (adaptive filters, its own deflate settings); [] without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return []
    import io
    rng = np.random.RandomState(3)
    rgb = _img(rng, 53, 37, 3)
    out = []
    for mode in ("RGB", "RGBA", "L", "LA", "P"):
        img = Image.fromarray(rgb, "RGB").convert(mode)
        for opt in (False, True):
            buf = io.BytesIO()
            img.save(buf, format="PNG", optimize=opt)
            want = np.asarray(img.convert("RGB")) if mode == "P" else (
                np.asarray(img)[..., :3] if mode in ("RGB", "RGBA") else np.repeat(np.asarray(img).reshape(37, 53, -1)[..., :1], 3, axis=2))
            out.append(("pillow-%s-%d" % (mode, opt), buf.getvalue(), np.ascontiguousarray(want)))
    buf = io.BytesIO()
    Image.fromarray(blob(224, 5), "RGB").save(buf, format="PNG")
    out.append(("pillow-blob", buf.getvalue(), blob(224, 5)))
    return out


# ---- malformed streams --------------------------------------------------------------------------------------------
MW, MH = 40, 30                                                  # every malformed stream claims to be a 40 x 30 image


def good_stream(ctype=2):
    """(w, h, ctype, palette, zlib bytes, expected pixels): a small good image, the neighbours of a malformed one."""
    arr = _img(np.random.RandomState(21), MW, MH, CHANNELS[ctype])
    return MW, MH, ctype, None, deflate(filter_rows(arr, ("seed", 6)), "l9"), expected(arr, ctype)


def malformed():
    """[(name, (w, h, ctype, palette, zlib bytes), expected status)]."""
    arr = _img(np.random.RandomState(22), MW, MH, 3)
    raw = filter_rows(arr, ("seed", 5))
    z = deflate(raw, "l9")
    assert (z[2] >> 1) & 3 == 2 and len(z) > 200                 # one dynamic block: byte 5 is inside its header
    out = []

    def add(name, zb, status, ctype=2, palette=None):
        out.append((name, (MW, MH, ctype, palette, bytes(zb)), status))
    for cut in (1, 5, len(z) // 2, len(z) - 5, len(z) - 2):
        add("cut-%d" % cut, z[:cut], TRUNCATED)
    add("block-type-3", b"\x78\x9c\x07\x00\x00\x00\x00\x00", BAD_BLOCK)
    add("stored-len-nlen", b"\x78\x01\x01\x05\x00\xfb\xff" + b"abcde" + b"\0\0\0\0", BAD_BLOCK)
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    b.lit(97)
    b.match(3, 2)
    b.lit(256)
    add("distance-past-start", zwrap(b.bytes(), b"a"), BAD_DISTANCE)
    add("one-byte-more", zlib.compress(raw + b"\0", 9), TOO_LONG)
    add("one-byte-less", zlib.compress(raw[:-1], 9), TOO_SHORT)
    add("adler-flip", z[:-1] + bytes([z[-1] ^ 1]), BAD_CHECKSUM)
    bad = bytearray(raw)
    bad[(1 + MW * 3) * 7] = 5
    add("filter-5", zlib.compress(bytes(bad), 9), BAD_FILTER)
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)                                              # nineteen code-length codes of one bit
    b.put(0, 32)
    add("oversubscribed", zwrap(b.bytes(), b""), BAD_CODES)
    flg = next(f for f in range(256) if f & 0x20 and (0x7800 + f) % 31 == 0)
    add("fdict", bytes([0x78, flg]) + z[2:], BAD_HEADER)
    idx = np.random.RandomState(23).randint(0, 2, size=(MH, MW, 1)).astype(np.uint8)
    idx[17, 23, 0] = 2
    add("palette-index", deflate(filter_rows(idx, 0), "l6"), BAD_PALETTE_INDEX, 3, np.array([[1, 2, 3], [4, 5, 6]], np.uint8))
    return out


def byte_flips(count, seed=0):
    """`count` copies of good streams with 1-3 bytes changed, seeded: (w, h, ctype, palette, zlib bytes)."""
    rng = np.random.RandomState(seed)
    base = [good_stream(c)[:5] for c in (0, 2, 4, 6)]
    arr = _img(np.random.RandomState(24), MW, MH, 3)
    base += [(MW, MH, 2, None, deflate(filter_rows(arr, "adaptive"), how)) for how in ("fixed", "stored", "l1", "flush", "w9")]
    for i in range(count):
        w, h, ctype, pal, z = base[i % len(base)]
        z = bytearray(z)
        for _ in range(int(rng.randint(1, 4))):
            z[int(rng.randint(0, len(z)))] = int(rng.randint(0, 256))
        yield w, h, ctype, pal, bytes(z)


# ---- the dump tests/native/png_core_check.cpp reads ---------------------------------------------------------------
def _record(w, h, ctype, palette, z, expect):
    pal = b"" if palette is None else np.ascontiguousarray(palette, np.uint8).tobytes()
    return struct.pack("<6i", w, h, ctype, len(pal) // 3, expect, len(z)) + pal + z


def dump(directory, flips=4000):
    """good.bin / malformed.bin / flips.bin: records of six int32 (w, h, colour type, palette entries, expected status or
    -1 for "any", stream bytes), the palette, the stream."""
    from gvcnn_tf_amd import records as R
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "good.bin"), "wb") as f:
        for _, png, _ in cases() + pillow_cases():
            w, h, ctype, pal, z = R.parse_png(png)
            f.write(_record(w, h, ctype, pal, z, OK))
    with open(os.path.join(directory, "malformed.bin"), "wb") as f:
        for _, (w, h, ctype, pal, z), status in malformed():
            f.write(_record(w, h, ctype, pal, z, status))
    with open(os.path.join(directory, "flips.bin"), "wb") as f:
        for w, h, ctype, pal, z in byte_flips(flips):
            f.write(_record(w, h, ctype, pal, z, -1))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4000)
