"""The batch PNG decoder on the host: gv_png_decode_host runs the decoder core of the device kernels (csrc/png_core.h)
serially, so everything but the kernels themselves is checked here, byte for byte (there is no tolerance): the case
matrix of tests/png_cases.py against records.decode_png and against the arrays the files were written from, the
malformed streams' status codes, the argument checks, and ViewBatcher(decode="device") on a CPU "device"."""
import ctypes as C
import os

import numpy as np
import pytest

import png_cases as PC
from gvcnn_tf_amd import _lib
from gvcnn_tf_amd import records as R

ALL = PC.cases()


@pytest.mark.parametrize("name,png,want", ALL, ids=[c[0] for c in ALL])
def test_host_decode_equals_decode_png_and_the_source_array(name, png, want):
    """parse_png + pack + gv_png_decode_host == decode_png == the array the file was written from."""
    ref = R.decode_png(png)
    assert ref.shape == want.shape and np.array_equal(ref, want)
    out, status = R.decode_png_batch_host([R.parse_png(png)])
    assert status.tolist() == [PC.OK]
    assert out.shape[1:] == want.shape and np.array_equal(out[0], want)


def test_pillow_files():
    pytest.importorskip("PIL.Image")
    for name, png, want in PC.pillow_cases():
        assert np.array_equal(R.decode_png(png), want), name
        out, status = R.decode_png_batch_host([R.parse_png(png)])
        assert status.tolist() == [PC.OK] and np.array_equal(out[0], want), name


def test_the_matrix_covers_every_block_type_filter_and_colour_type():
    """Nothing depends on the Pillow files: the numpy-written cases alone hold stored, fixed and dynamic blocks, the five
    filter types and the five colour types."""
    import zlib
    btypes, filters, ctypes_seen = set(), set(), set()
    for _, png, _ in ALL:
        w, h, ctype, _, z = R.parse_png(png)
        ctypes_seen.add(ctype)
        btypes.add((z[2] >> 1) & 3)
        raw = np.frombuffer(zlib.decompress(z), np.uint8).reshape(h, -1)
        filters |= set(raw[:, 0].tolist())
    assert btypes == {0, 1, 2} and filters == {0, 1, 2, 3, 4} and ctypes_seen == {0, 2, 3, 4, 6}


def test_parse_png_walks_the_chunks_like_decode_png():
    name, png, _ = ALL[1]
    w, h, ctype, pal, z = R.parse_png(png)
    assert (w, h, ctype, pal) == (3, 5, 2, None)
    import zlib
    assert len(zlib.decompress(z)) == h * (1 + w * 3)
    with pytest.raises(ValueError, match="not a PNG"):
        R.parse_png(b"nope" + png)
    sixteen = bytearray(png)
    sixteen[24] = 16                                             # IHDR bit depth
    with pytest.raises(ValueError, match="only 8-bit non-interlaced"):
        R.parse_png(bytes(sixteen))
    laced = bytearray(png)
    laced[28] = 1                                                # IHDR interlace method
    with pytest.raises(ValueError, match="only 8-bit non-interlaced"):
        R.parse_png(bytes(laced))


def test_mixed_batch_of_seventy():
    """One call, 70 images of one size: stream lengths, colour types, filters and deflate variants mixed."""
    rng = np.random.RandomState(1)
    pal = rng.randint(0, 256, size=(200, 3)).astype(np.uint8)
    pngs, want = [], []
    hows = list(PC.DEFLATE)
    for i in range(70):
        ctype = (0, 2, 3, 4, 6)[i % 5]
        arr = PC._img(rng, 21, 9, PC.CHANNELS[ctype])
        if ctype == 3:
            arr = arr % 200
        pngs.append(R.parse_png(PC.write_png(arr, ctype, pal if ctype == 3 else None, filters=("seed", i), how=hows[i % len(hows)])))
        want.append(PC.expected(arr, ctype, pal))
    out, status = R.decode_png_batch_host(pngs)
    assert not status.any() and np.array_equal(out, np.stack(want))


BAD = PC.malformed()


@pytest.mark.parametrize("name,stream,want", BAD, ids=[b[0] for b in BAD])
def test_malformed_stream_between_two_good_images(name, stream, want):
    """The status is the expected non-zero one, the neighbours are right, the call itself returns 0."""
    good = PC.good_stream()
    out, status = R.decode_png_batch_host([good[:5], stream, good[:5]])
    assert status.tolist() == [PC.OK, want, PC.OK]
    assert np.array_equal(out[0], good[5]) and np.array_equal(out[2], good[5])


def test_argument_checks():
    lib = _lib.load()
    good = PC.good_stream()
    buf, images, (h0, w0) = R.pack_png_batch([good[:5]])
    out, status = np.empty((1, h0, w0, 3), np.uint8), np.empty(1, np.int32)

    def call(b=buf, nbytes=None, im=images, n=1, o=out, s=status, pal=None):
        return lib.gv_png_decode_host(b.ctypes.data if b is not None else None, b.size if nbytes is None else nbytes, im, n, h0,
                                      w0, pal, o.ctypes.data if o is not None else None, s.ctypes.data if s is not None else None)
    assert call() == 0 and status[0] == 0
    assert call(b=None, nbytes=buf.size) == _lib.GV_E_BADARG and call(o=None) == _lib.GV_E_BADARG
    assert call(s=None) == _lib.GV_E_BADARG and call(im=None) == _lib.GV_E_BADARG
    assert call(n=0) == _lib.GV_E_BADARG and call(n=-3) == _lib.GV_E_BADARG
    assert call(nbytes=images[0].length + 15) == _lib.GV_E_BADARG          # the stream runs into the 16 bytes of padding
    assert call(nbytes=images[0].length + 16) == 0
    for field, value in (("offset", 8), ("color_type", 1), ("color_type", 5), ("length", -1)):
        im = (_lib.PngImage * 1)()
        C.memmove(im, images, C.sizeof(im))
        setattr(im[0], field, value)
        assert call(im=im) == _lib.GV_E_BADARG, field
    im = (_lib.PngImage * 1)()
    C.memmove(im, images, C.sizeof(im))
    im[0].color_type, im[0].palette_len = 3, 2
    assert call(im=im) == _lib.GV_E_BADARG                                  # a palette image without `palettes`
    im[0].palette_len = 257
    assert call(im=im, pal=buf.ctypes.data) == _lib.GV_E_BADARG
    assert lib.gv_png_decode_workspace_bytes(0, 100) == _lib.GV_E_BADARG and lib.gv_png_decode_workspace_bytes(2, 0) == _lib.GV_E_BADARG
    assert lib.gv_png_decode_workspace_bytes(3, 100) == 80 + 3 * 112
    assert lib.gv_png_decode_batch(None, 0, None, 0, 0, 0, None, None, None, None, 0, None) == _lib.GV_E_BADARG


# ---- ViewBatcher(decode="device") on a CPU "device" ---------------------------------------------------------------
def _write(path, shapes, filters):
    R.write_tfrecords(path, [R.make_example([PC.write_png(v, 2, filters=filters) for v in views], lab) for views, lab in shapes])


@pytest.fixture(scope="module")
def record_files(tmp_path_factory):
    rng = np.random.RandomState(4)
    shapes = [([PC._img(rng, 16, 12, 3) for _ in range(3)], k) for k in range(23)]
    d = tmp_path_factory.mktemp("png_records")
    one, a, b = (os.path.join(d, n) for n in ("one.record", "a.record", "b.record"))
    _write(one, shapes, ("seed", 1))
    _write(a, shapes[:9], 4)
    _write(b, shapes[9:], "adaptive")
    return one, [a, b]


def _same_shapes(path, **kw):
    host = list(R.ViewBatcher(path, 3, 8, 8, 4, "cpu", decode="host", **kw)._shapes())
    dev = list(R.ViewBatcher(path, 3, 8, 8, 4, "cpu", decode="device", **kw)._shapes())
    assert len(host) == len(dev) == 23
    for (a, la), (b, lb) in zip(host, dev):
        assert la == lb and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_batcher_device_mode_yields_the_host_mode_shapes(record_files):
    one, two = record_files
    _same_shapes(one)
    _same_shapes(two)
    _same_shapes(one, seed=5, shuffle_buffer=8)
    _same_shapes(two, seed=6, shuffle_buffer=5, remainder="pad")
    _same_shapes(one, remainder="pad")
    with pytest.raises(ValueError, match="decode must be"):
        R.ViewBatcher(one, 3, 8, 8, 4, "cpu", decode="gpu")


def test_batcher_pads_parsed_records_like_decoded_ones(record_files, monkeypatch):
    """remainder="pad" through __iter__: the batches of parsed records (what the device decodes) hold the records the
    host path's batches hold, the last one padded with its last real shape."""
    one, _ = record_files
    seen = []
    vb = R.ViewBatcher(one, 3, 8, 8, 4, "cpu", decode="device", remainder="pad")
    monkeypatch.setattr(vb, "_batch_device", lambda items, labels: seen.append(([k for _, k in items], list(labels))))
    assert len(list(vb)) == 6 and vb.last_valid == 3
    assert seen[0] == ([0, 1, 2, 3], [0, 1, 2, 3]) and seen[-1] == ([20, 21, 22, 22], [20, 21, 22, -1])


def test_corrupt_view_raises_naming_record_and_view(tmp_path):
    rng = np.random.RandomState(8)
    shapes = [([PC._img(rng, 16, 12, 3) for _ in range(3)], k) for k in range(6)]
    recs = []
    for k, (views, lab) in enumerate(shapes):
        enc = [PC.write_png(v, 2, filters=1) for v in views]
        if k == 4:
            w, h, ctype, pal, z = R.parse_png(enc[1])
            enc[1] = PC.wrap_png(w, h, ctype, z[:-1] + bytes([z[-1] ^ 0x40]))
        recs.append(R.make_example(enc, lab))
    path = os.path.join(tmp_path, "bad.record")
    R.write_tfrecords(path, recs)
    with pytest.raises(ValueError, match=r"record 4 view 1: GV_PNG_BAD_CHECKSUM"):
        list(R.ViewBatcher(path, 3, 8, 8, 2, "cpu", decode="device")._shapes())
