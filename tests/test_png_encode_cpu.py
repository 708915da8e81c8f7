"""The PNG encoder's host twin (gv_png_encode_host: the encoder core of csrc/png_enc_core.h run serially) against a numpy
restatement of the line filters (the filtered bytes, exactly) and zlib / the project's decoders / Pillow (the stream).
No GPU.  The size conditions are caps derived from the format and from the inputs (each derivation at its test): a
stored-only or literal-only encoder does not pass them."""
import heapq
import struct
import zlib

import numpy as np
import pytest

import png_enc_cases as EC
from gvcnn_tf_amd import _lib
from gvcnn_tf_amd import records as R

IMAGES = EC.images()
NAMES = [n for n, _ in IMAGES]
BY_NAME = dict(IMAGES)
_STREAMS = {}


def stream(name, filt, color):
    """(zlib stream, colour type) of a case, encoded once and shared"""
    key = (name, filt, color)
    if key not in _STREAMS:
        _STREAMS[key] = EC.stream(BY_NAME[name], filt, color)
    return _STREAMS[key]


def segments(raw_len):
    return -(-raw_len // EC.seg_bytes())


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_segment_size_and_bound(lib):
    SEG = lib.gv_png_encode_segment_bytes()
    assert SEG in (8192, 16384)
    for name, img in IMAGES:
        h, w, _ = img.shape
        raw, bound = h * (1 + 3 * w), lib.gv_png_encode_bound(h, w)
        assert bound % 16 == 0
        # a stored block and a sync marker cost 10 bytes per segment of at least 4 KB
        assert 2 + raw + 10 * segments(raw) + 4 <= bound <= raw + raw // 8 + 64, name


@pytest.mark.parametrize("name", NAMES)
def test_round_trip(lib, name):
    img = BY_NAME[name]
    h, w, _ = img.shape
    for filt in EC.FILTERS:
        for color in EC.COLORS:
            z, ctype = stream(name, filt, color)
            ch = 1 if ctype == 0 else 3
            d = zlib.decompressobj()
            raw = d.decompress(z)
            assert d.eof and not d.unused_data and len(raw) == h * (1 + w * ch)      # (eof: the Adler-32 was accepted)
            assert z[:2] == b"\x78\x01" and struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
            assert len(z) <= lib.gv_png_encode_bound(h, w)
            png = R.png_from_stream(w, h, ctype, z)
            assert np.array_equal(R.decode_png(png), img), (filt, color)
            out, status = R.decode_png_batch_host([R.parse_png(png)])
            assert status.tolist() == [_lib.GV_PNG_OK] and np.array_equal(out[0], img), (filt, color)


def test_pillow_opens_the_files():
    Image = pytest.importorskip("PIL.Image")
    import io
    for name in NAMES:
        img = BY_NAME[name]
        for filt, color in ((EC.ADAPTIVE, EC.AUTO), (4, EC.RGB)):
            z, ctype = stream(name, filt, color)
            im = Image.open(io.BytesIO(R.png_from_stream(img.shape[1], img.shape[0], ctype, z)))
            assert im.mode == ("L" if ctype == 0 else "RGB")
            assert np.array_equal(np.asarray(im.convert("RGB")), img), name


@pytest.mark.parametrize("name", NAMES)
def test_filter_bytes_and_filtered_rows_equal_the_numpy_restatement(name):
    img = BY_NAME[name]
    for filt in EC.FILTERS:
        for color in EC.COLORS:
            z, ctype = stream(name, filt, color)
            want_type, types, raw = EC.expected_raw(img, filt, color)
            assert ctype == want_type
            got = np.frombuffer(zlib.decompress(z), np.uint8).reshape(raw.shape)
            if filt != EC.ADAPTIVE:
                assert (got[:, 0] == filt).all()
            assert np.array_equal(got[:, 0], types), "filter type per row"
            assert np.array_equal(got, raw)


def test_adaptive_tie_takes_the_lowest_type():
    img = EC.constant(4, 2, 5)
    cost = EC.filter_costs(EC.filter_candidates(img[..., 0].reshape(2, 4), 1))
    # row 0: Sub and Paeth tie below the rest; row 1: Up and Paeth tie at zero
    assert cost[1, 0] == cost[4, 0] < min(cost[0, 0], cost[2, 0], cost[3, 0])
    assert cost[2, 1] == cost[4, 1] == 0 < min(cost[0, 1], cost[1, 1], cost[3, 1])
    z, ctype = EC.stream(img)
    assert ctype == 0 and np.frombuffer(zlib.decompress(z), np.uint8).reshape(2, 5)[:, 0].tolist() == [1, 2]
    z, _ = EC.stream(EC.constant(6, 3, 0))                       # every cost is 0 on every row
    assert np.frombuffer(zlib.decompress(z), np.uint8).reshape(3, 7)[:, 0].tolist() == [0, 0, 0]


def test_colour_type():
    for name, img in IMAGES:
        gray = bool((img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all())
        assert stream(name, EC.ADAPTIVE, EC.AUTO)[1] == (0 if gray else 2), name
        assert stream(name, EC.ADAPTIVE, EC.RGB)[1] == 2, name
        if "first-pixel" in name or "last-pixel" in name:
            assert not gray and stream(name, 0, EC.AUTO)[1] == 2
    assert sum("pixel" in n for n in NAMES) >= 4


# ---- size conditions ------------------------------------------------------------------------------------------------
def test_size_constant_image():
    """Forced filter 2 on a constant gray image: every row is its filter byte and 224 equal bytes (zeros from row 1 on).
    Runs coded as matches take at most ceil(SEG / 258) matches of no more than 12 bits under the fixed code per
    segment, plus block overhead: 128 bytes a segment are ample, plus header and trailer."""
    SEG = EC.seg_bytes()
    for v in (0, 77):
        z, ctype = EC.stream(EC.constant(224, 224, v), 2, EC.AUTO)
        assert ctype == 0
        assert len(z) <= 128 * segments(224 * 225) + 6, len(z)
    assert -(-SEG // 258) * 12 // 8 < 100


def _huffman_depths(counts):
    heap = [(c, i, (i,)) for i, c in enumerate(counts) if c]
    depth = dict.fromkeys((i for _, i, _ in heap), 0)
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return depth


def _segment_spans(z, raw_len):
    """[(first, behind)] byte spans of the segments of a stream: inflate byte by byte, a segment's bytes are consumed
    when the output reaches its end; the sync marker 00 00 FF FF behind it closes the span"""
    SEG, d, got, ends = EC.seg_bytes(), zlib.decompressobj(), 0, []
    for i in range(len(z)):
        got += len(d.decompress(z[i:i + 1]))
        while len(ends) < segments(raw_len) - 1 and got >= (len(ends) + 1) * SEG:
            ends.append(z.index(b"\x00\x00\xff\xff", i) + 4)
    assert d.eof and got == raw_len
    cuts = [2] + ends + [len(z) - 4]
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("w,h", [(150, 120), (127, 64), (100, 40)], ids=["three-segments", "exactly-one", "short"])
def test_size_run_free_image(w, h):
    """Gray, forced filter 0, no byte equal to its left neighbour: literals only, so what is left to win is the entropy
    code.  Per segment the bits stay under n (H + p_max + 0.086) — the classical bound on the redundancy of a Huffman
    code — + 2400 (the largest dynamic header) + 40 (the sync block); the sample's optimal code needs no more than 15
    bits (asserted), so the length limit costs nothing.  zlib's own Huffman-only coder is held to the same bound first."""
    SEG = EC.seg_bytes()
    img = EC.run_free(w, h, 3)
    z, ctype = EC.stream(img, 0, EC.AUTO)
    raw = zlib.decompress(z)
    assert ctype == 0 and len(raw) == h * (1 + w) and all(raw[i] != raw[i - 1] for i in range(1, len(raw)))
    spans = _segment_spans(z, len(raw))
    assert len(spans) == segments(len(raw))
    for s, (a, b) in enumerate(spans):
        part = raw[s * SEG:(s + 1) * SEG]
        counts = np.bincount(np.frombuffer(part, np.uint8), minlength=256)
        assert max(_huffman_depths(list(counts) + [1]).values()) <= 15          # (+ the end-of-block symbol)
        p = counts[counts > 0] / len(part)
        bound = len(part) * (-(p * np.log2(p)).sum() + p.max() + 0.086) + 2400 + 40
        co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        ref = co.compress(part) + co.flush(zlib.Z_SYNC_FLUSH)
        print("segment %d: %d bytes, entropy bound %.0f bits, zlib %d bits, encoder %d bits" % (s, len(part), bound, 8 * len(ref), 8 * (b - a)))
        assert 8 * len(ref) <= bound
        assert 8 * (b - a) <= bound, (s, 8 * (b - a), bound)


def test_size_noise_falls_back_to_stored():
    img = EC.rgb_noise(224, 224, 8)
    for filt in (0, EC.ADAPTIVE):
        z, ctype = EC.stream(img, filt, EC.AUTO)
        raw = 224 * (1 + 3 * 224)
        assert ctype == 2 and len(z) <= raw + 10 * segments(raw) + 6


# ---- batches --------------------------------------------------------------------------------------------------------
def test_mixed_batch_of_seventy():
    views = EC.mixed_batch()
    rc, out, length, ctype = EC.encode_host(views)
    assert rc == 0 and set(ctype.tolist()) == {0, 2}
    for i in range(len(views)):
        z, ct = EC.stream(views[i])
        assert out[i, :length[i]].tobytes() == z and ctype[i] == ct, i
        assert (out[i, length[i]:] == 0xA5).all()


def test_two_calls_give_identical_bytes():
    views = np.stack([EC.disc(100, 100), EC.one_pixel(100, 100, "last")])
    a, b = EC.encode_host(views), EC.encode_host(views)
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_argument_checks(lib):
    views = EC.mixed_batch(2)
    n, h, w, _ = views.shape
    bound = lib.gv_png_encode_bound(h, w)
    out = np.full((n, bound + 16), 0xA5, np.uint8)
    length, ctype = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    ws_bytes = lib.gv_png_encode_workspace_bytes(n, h, w)
    assert ws_bytes > 0
    ws = np.zeros(ws_bytes + 32, np.uint8)
    ws_ptr = (ws.ctypes.data + 15) // 16 * 16
    good = dict(src=views.ctypes.data, n=n, h0=h, w0=w, filter=EC.ADAPTIVE, color=EC.AUTO, out=out.ctypes.data, out_stride=bound,
                length=length.ctypes.data, color_type=ctype.ctypes.data)
    order = ("src", "n", "h0", "w0", "filter", "color", "out", "out_stride", "length", "color_type")

    def host(**kw):
        a = dict(good, **kw)
        return lib.gv_png_encode_host(*[a[k] for k in order])

    def batch(ws=ws_ptr, ws_bytes=ws_bytes, **kw):
        # (argument errors come back before any HIP call: host memory and no device will do)
        a = dict(good, **kw)
        return lib.gv_png_encode_batch(*[a[k] for k in order], ws, ws_bytes, None)
    for call in (host, batch):
        for bad in (dict(src=None), dict(out=None), dict(length=None), dict(color_type=None), dict(n=0), dict(h0=0), dict(w0=-1),
                    dict(filter=6), dict(filter=-1), dict(color=2), dict(color=-1), dict(out_stride=bound - 16),
                    dict(out_stride=bound + 8)):
            assert call(**bad) == _lib.GV_E_BADARG, (call.__name__, bad)
        assert call(h0=50000, w0=50000, out_stride=1 << 40) == _lib.GV_E_UNSUPPORTED
    assert batch(ws=None) == _lib.GV_E_BADARG and batch(ws_bytes=ws_bytes - 1) == _lib.GV_E_BADARG
    assert batch(ws=ws_ptr + 4) == _lib.GV_E_ALIGN
    assert lib.gv_png_encode_bound(0, 5) == _lib.GV_E_BADARG and lib.gv_png_encode_bound(50000, 50000) == _lib.GV_E_UNSUPPORTED
    assert lib.gv_png_encode_workspace_bytes(0, 4, 4) == _lib.GV_E_BADARG
    assert (out == 0xA5).all() and (length == -7).all() and (ctype == -7).all() and not ws.any()
    assert host(out_stride=bound + 16) == 0 and (length > 0).all()


# ---- Python ---------------------------------------------------------------------------------------------------------
def test_encode_png_batch_on_numpy():
    views = EC.mixed_batch(9)
    for filt, fc, color, cc in (("adaptive", EC.ADAPTIVE, "auto", EC.AUTO), (4, 4, "rgb", EC.RGB), ("up", 2, "auto", EC.AUTO)):
        rc, out, length, ctype = EC.encode_host(views, fc, cc)
        want = [R.png_from_stream(views.shape[2], views.shape[1], ctype[i], out[i, :length[i]].tobytes()) for i in range(9)]
        got = R.encode_png_batch(views, filter=filt, color=color)
        assert got == want and all(isinstance(p, bytes) for p in got)
        for p, v in zip(got, views):
            assert np.array_equal(R.decode_png(p), v)
    with pytest.raises(ValueError):
        R.encode_png_batch(views, filter="best")
    with pytest.raises(ValueError):
        R.encode_png_batch(views, color="gray")


def test_png_from_stream_layout():
    z = zlib.compress(b"\0abc")
    png = R.png_from_stream(1, 1, 2, z)
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR" and png[16:29] == struct.pack(">IIBBBBB", 1, 1, 8, 2, 0, 0, 0)
    assert R.parse_png(png) == (1, 1, 2, None, z) and png.count(b"IDAT") == 1 and png.endswith(b"IEND\xaeB`\x82")


def test_encode_png_is_unchanged():
    img = EC.disc(37, 23)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(23))
    want = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 37, 23, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    assert R.encode_png(img) == want
