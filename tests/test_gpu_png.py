"""The batch PNG decoder on the device (gv_png_decode_batch: inflate + un-filter + expand kernels of csrc/png.hip)
against records.decode_png and the arrays the files were written from, byte for byte; the case matrix, the malformed
streams and the record files are those of the CPU file (tests/png_cases.py), where the same streams run through the
same decoder core on the host first.

Guards: `out` is allocated with a row of a known byte in front of and behind the image slots of a call and the workspace
with 256 such bytes on either side; every call checks them.  (The slots of one call are contiguous by the ABI — the
cases of the matrix have different sizes and so are one call each, slot and guards; in a batch a stray write into a
neighbour shows as a wrong byte of that neighbour.)"""
import os

import numpy as np
import pytest
import torch

import png_cases as PC
from gvcnn_tf_amd import _lib
from gvcnn_tf_amd import records as R

pytestmark = pytest.mark.gpu
GUARD = 256


def device_decode(pngs):
    """parse_png results of one size -> (rc, out uint8 [n, h0, w0, 3], status [n]); asserts every guard."""
    from gvcnn_tf_amd.model import _st
    lib, dev = _lib.load(), torch.device("cuda:0")
    buf, images, (h0, w0) = R.pack_png_batch(pngs)
    n, row = len(pngs), w0 * 3
    streams = torch.from_numpy(buf).to(dev)
    out = torch.full((row + n * h0 * row + row,), 0xA5, dtype=torch.uint8, device=dev)
    ws_bytes = lib.gv_png_decode_workspace_bytes(n, h0 * (1 + 4 * w0))
    assert ws_bytes > 0
    ws = torch.full((GUARD + ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.full((n + 2,), -77, dtype=torch.int32, device=dev)
    assert (ws.data_ptr() + GUARD) % 16 == 0
    rc = lib.gv_png_decode_batch(streams.data_ptr(), buf.size, images, n, h0, w0, streams.data_ptr(), out.data_ptr() + row,
                                 status.data_ptr() + 4, ws.data_ptr() + GUARD, ws_bytes, _st())
    torch.cuda.synchronize()
    out, ws, status = out.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    assert (out[:row] == 0xA5).all() and (out[-row:] == 0xA5).all(), "guard row of out"
    assert (ws[:GUARD] == 0x5A).all() and (ws[-GUARD:] == 0x5A).all(), "guard of the workspace"
    assert status[0] == -77 and status[-1] == -77, "guard of status"
    assert np.array_equal(streams.cpu().numpy(), buf), "the input was written to"
    return rc, out[row:-row].reshape(n, h0, w0, 3), status[1:-1]


ALL = PC.cases()


@pytest.mark.parametrize("name,png,want", ALL, ids=[c[0] for c in ALL])
def test_case_matrix(name, png, want):
    assert np.array_equal(R.decode_png(png), want)
    rc, out, status = device_decode([R.parse_png(png)])
    assert rc == 0 and status.tolist() == [PC.OK]
    assert out.shape[1:] == want.shape and np.array_equal(out[0], want)


def test_pillow_files():
    pytest.importorskip("PIL.Image")
    for name, png, want in PC.pillow_cases():
        assert np.array_equal(R.decode_png(png), want), name
        rc, out, status = device_decode([R.parse_png(png)])
        assert rc == 0 and status.tolist() == [PC.OK] and np.array_equal(out[0], want), name


def test_mixed_batch_of_seventy():
    """n = 70 in one call: stream lengths, colour types, filters and deflate variants mixed; and the host twin agrees."""
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
    rc, out, status = device_decode(pngs)
    assert rc == 0 and not status.any() and np.array_equal(out, np.stack(want))
    host, hstatus = R.decode_png_batch_host(pngs)
    assert np.array_equal(host, out) and np.array_equal(hstatus, status)


BAD = PC.malformed()


@pytest.mark.parametrize("name,stream,want", BAD, ids=[b[0] for b in BAD])
def test_malformed_stream_between_two_good_images(name, stream, want):
    """Error paths of a bounds-checked decoder (each of these streams went through gv_png_decode_host first, in the CPU
    file and under the stand-alone sanitizer build): the expected status, exact neighbours, untouched guards, rc 0."""
    good = PC.good_stream()
    _, hstatus = R.decode_png_batch_host([good[:5], stream, good[:5]])
    assert hstatus.tolist() == [PC.OK, want, PC.OK]
    rc, out, status = device_decode([good[:5], stream, good[:5]])
    assert rc == 0 and status.tolist() == [PC.OK, want, PC.OK]
    assert np.array_equal(out[0], good[5]) and np.array_equal(out[2], good[5])


def test_argument_checks_on_device_pointers():
    from gvcnn_tf_amd.model import _st
    lib, dev = _lib.load(), torch.device("cuda:0")
    good = PC.good_stream()
    buf, images, (h0, w0) = R.pack_png_batch([good[:5]])
    streams = torch.from_numpy(buf).to(dev)
    out = torch.zeros(h0 * w0 * 3, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.gv_png_decode_workspace_bytes(1, h0 * (1 + 4 * w0))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=dev)

    def call(n=1, ws_ptr=ws.data_ptr(), ws_bytes=need, nbytes=buf.size):
        return lib.gv_png_decode_batch(streams.data_ptr(), nbytes, images, n, h0, w0, None, out.data_ptr(), status.data_ptr(),
                                       ws_ptr, ws_bytes, _st())
    assert call(n=0) == _lib.GV_E_BADARG and call(ws_ptr=None) == _lib.GV_E_BADARG
    assert call(ws_bytes=need - 1) == _lib.GV_E_BADARG and call(ws_ptr=ws.data_ptr() + 4) == _lib.GV_E_ALIGN
    assert call(nbytes=images[0].length + 15) == _lib.GV_E_BADARG
    assert call() == 0
    torch.cuda.synchronize()
    assert status.item() == 0 and np.array_equal(out.cpu().numpy().reshape(h0, w0, 3), good[5])


# ---- end to end: ViewBatcher(decode="device") == ViewBatcher(decode="host"), bit for bit -----------------------------
@pytest.fixture(scope="module")
def record_files(tmp_path_factory):
    rng = np.random.RandomState(4)
    shapes = [([PC._img(rng, 16, 12, 3) for _ in range(3)], k) for k in range(9)]

    def write(path, part, filters):
        R.write_tfrecords(path, [R.make_example([PC.write_png(v, 2, filters=filters) for v in views], lab) for views, lab in part])
    d = tmp_path_factory.mktemp("png_records")
    one, a, b = (os.path.join(d, n) for n in ("one.record", "a.record", "b.record"))
    write(one, shapes, ("seed", 1))
    write(a, shapes[:3], 4)
    write(b, shapes[3:], "adaptive")
    return one, [a, b]


def _batches(path, decode, **kw):
    vb = R.ViewBatcher(path, 3, 8, 8, 2, "cuda:0", decode=decode, **kw)
    out = [(x.cpu().numpy(), y.numpy()) for x, y in vb]
    return out, vb.last_valid, vb.dropped


@pytest.mark.parametrize("which,kw", [("one", dict(augment=True, seed=3)), ("one", dict()),
                                      ("one", dict(augment=True, seed=5, shuffle_buffer=4)),
                                      ("one", dict(remainder="pad")), ("two", dict(augment=True, seed=7, remainder="pad"))],
                         ids=["augment", "plain", "shuffle", "pad", "two-files"])
def test_batcher_device_mode_equals_host_mode(record_files, which, kw):
    import warnings
    path = record_files[0] if which == "one" else record_files[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # (the dropped-remainder warning of both modes)
        host, hv, hd = _batches(path, "host", **kw)
        dev, dv, dd = _batches(path, "device", **kw)
    assert len(host) == len(dev) == (5 if kw.get("remainder") == "pad" else 4) and (hv, hd) == (dv, dd)
    for (xa, ya), (xb, yb) in zip(host, dev):
        assert xa.shape == xb.shape == (2, 3, 8, 8, 3) and np.array_equal(xa, xb) and np.array_equal(ya, yb)


def test_corrupt_view_raises_no_later_than_the_following_batch(tmp_path):
    rng = np.random.RandomState(8)
    recs = []
    for k in range(8):
        enc = [PC.write_png(PC._img(rng, 16, 12, 3), 2, filters=1) for _ in range(3)]
        if k == 3:                                               # second record of batch 1
            w, h, ctype, pal, z = R.parse_png(enc[2])
            enc[2] = PC.wrap_png(w, h, ctype, z[:-1] + bytes([z[-1] ^ 0x40]))
        recs.append(R.make_example(enc, k))
    path = os.path.join(tmp_path, "bad.record")
    R.write_tfrecords(path, recs)
    got = 0
    with pytest.raises(ValueError, match=r"record 3 view 2: GV_PNG_BAD_CHECKSUM"):
        for _ in R.ViewBatcher(path, 3, 8, 8, 2, "cuda:0", decode="device"):
            got += 1
    assert 1 <= got <= 2                                         # batch 0 is good; batch 1 may come out, batch 2 never does
