"""The batch PNG encoder on the device (gv_png_encode_batch: colour, filter, segment and gather kernels of
csrc/png_enc.hip) against its host twin (gv_png_encode_host: the same core, run serially), byte for byte — the twin
itself is held to the numpy filters, zlib and the size caps in tests/test_png_encode_cpu.py — then device to device
through the decoder, through ViewRenderer.render_png and through a record file.

Guards: `out` is allocated with a slot of a known byte in front of and behind the slots of a call, the workspace with
256 such bytes on either side, `length` and `color_type` with a guard element on either side; every call checks them,
that no slot is written past its length, and that `src` is unchanged."""
import os

import numpy as np
import pytest
import torch

import png_enc_cases as EC
from gvcnn_tf_amd import _lib
from gvcnn_tf_amd import records as R
from gvcnn_tf_amd import render

pytestmark = pytest.mark.gpu
GUARD = 256
DEV = torch.device("cuda:0")


def device_encode(views, filt=EC.ADAPTIVE, color=EC.AUTO, stream=None):
    """uint8 [n, h, w, 3] -> (rc, out uint8 [n, bound], length [n], colour type [n]); asserts every guard."""
    from gvcnn_tf_amd.model import _st
    lib = _lib.load()
    views = np.ascontiguousarray(views, np.uint8)
    n, h, w, _ = views.shape
    stride = lib.gv_png_encode_bound(h, w)
    src = torch.from_numpy(views).to(DEV)
    out = torch.full(((n + 2) * stride,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_bytes = lib.gv_png_encode_workspace_bytes(n, h, w)
    assert ws_bytes > 0
    ws = torch.full((GUARD + ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    length = torch.full((n + 2,), -77, dtype=torch.int32, device=DEV)
    ctype = torch.full((n + 2,), -77, dtype=torch.int32, device=DEV)
    assert (ws.data_ptr() + GUARD) % 16 == 0 and (out.data_ptr() + stride) % 16 == 0
    torch.cuda.synchronize()
    rc = lib.gv_png_encode_batch(src.data_ptr(), n, h, w, filt, color, out.data_ptr() + stride, stride, length.data_ptr() + 4,
                                 ctype.data_ptr() + 4, ws.data_ptr() + GUARD, ws_bytes, _st() if stream is None else stream)
    torch.cuda.synchronize()
    out, ws, length, ctype = out.cpu().numpy().reshape(n + 2, stride), ws.cpu().numpy(), length.cpu().numpy(), ctype.cpu().numpy()
    assert (out[0] == 0xA5).all() and (out[-1] == 0xA5).all(), "guard slot of out"
    assert (ws[:GUARD] == 0x5A).all() and (ws[-GUARD:] == 0x5A).all(), "guard of the workspace"
    assert length[0] == length[-1] == -77 and ctype[0] == ctype[-1] == -77, "guard of length / color_type"
    assert np.array_equal(src.cpu().numpy(), views), "the input was written to"
    out, length, ctype = out[1:-1], length[1:-1], ctype[1:-1]
    if rc == 0:
        for i in range(n):
            assert 6 <= length[i] <= stride and (out[i, length[i]:] == 0xA5).all(), "slot %d written past its length" % i
    return rc, out, length, ctype


def assert_same_as_host(views, filt, color, got):
    rc, out, length, ctype = got
    hrc, hout, hlength, hctype = EC.encode_host(views, filt, color)
    assert rc == 0 and hrc == 0
    assert np.array_equal(length, hlength) and np.array_equal(ctype, hctype)
    assert np.array_equal(out, hout)                             # (both pre-filled with 0xA5 past the lengths)


IMAGES = EC.images()


@pytest.mark.parametrize("name,img", IMAGES, ids=[n for n, _ in IMAGES])
def test_case_matrix(name, img):
    for filt in (EC.ADAPTIVE, 4):
        for color in EC.COLORS:
            assert_same_as_host(img[None], filt, color, device_encode(img[None], filt, color))


def test_mixed_batch_of_seventy():
    views = EC.mixed_batch()
    for filt, color in ((EC.ADAPTIVE, EC.AUTO), (4, EC.RGB)):
        assert_same_as_host(views, filt, color, device_encode(views, filt, color))


def test_device_to_device_round_trip():
    from gvcnn_tf_amd.model import _st
    lib = _lib.load()
    views = np.concatenate([EC.mixed_batch(14, 100, 100), np.stack([EC.disc(100, 100), EC.rgb_noise(100, 100, 3)])])
    n, h, w, _ = views.shape
    stride = lib.gv_png_encode_bound(h, w)
    src = torch.from_numpy(views).to(DEV)
    streams = torch.zeros(n * stride + 16, dtype=torch.uint8, device=DEV)
    info = torch.zeros((2, n), dtype=torch.int32, device=DEV)
    ws_bytes = lib.gv_png_encode_workspace_bytes(n, h, w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert lib.gv_png_encode_batch(src.data_ptr(), n, h, w, EC.ADAPTIVE, EC.AUTO, streams.data_ptr(), stride, info[0].data_ptr(),
                                   info[1].data_ptr(), ws.data_ptr(), ws_bytes, _st()) == 0
    length, ctype = info.cpu().numpy()
    images = (_lib.PngImage * n)()
    for i in range(n):                                           # the slots are 16-byte aligned: the decoder reads them in place
        images[i].offset, images[i].length, images[i].color_type = i * stride, int(length[i]), int(ctype[i])
    dws_bytes = lib.gv_png_decode_workspace_bytes(n, h * (1 + 4 * w))
    dws = torch.empty(dws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert lib.gv_png_decode_batch(streams.data_ptr(), streams.numel(), images, n, h, w, None, out.data_ptr(), status.data_ptr(),
                                   dws.data_ptr(), dws_bytes, _st()) == 0
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and set(ctype.tolist()) == {0, 2}
    assert np.array_equal(out.cpu().numpy(), views)


def _cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * 0.7 + [0.3, -0.2, 0.1]
    t = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return v, np.array(t, np.int32)


def test_render_png():
    r = render.ViewRenderer(2, 32, 32, device=DEV, color=(0.6, 0.6, 0.6))       # a gray surface on the white background
    meshes = [render.icosphere(0), _cube()]
    want = r.render_uint8(meshes).cpu().numpy()
    status = r.status.copy()
    r.status = None
    pngs = r.render_png(meshes)
    assert np.array_equal(r.status, status) and len(pngs) == 2 and all(len(p) == 2 for p in pngs)
    for i in range(2):
        for v in range(2):
            w, h, ctype, _, _ = R.parse_png(pngs[i][v])
            assert (w, h, ctype) == (32, 32, 0)
            assert np.array_equal(R.decode_png(pngs[i][v]), want[i, v])
    assert want.min() < want.max()
    again = r.render_png(meshes, filter="paeth", color="rgb")
    assert R.parse_png(again[1][1])[2] == 2 and np.array_equal(R.decode_png(again[1][1]), want[1, 1])
    blue = render.ViewRenderer(2, 32, 32, device=DEV)            # the default surface colour is not gray: colour type 2
    want = blue.render_uint8(meshes).cpu().numpy()
    pngs = blue.render_png(meshes)
    for i in range(2):
        for v in range(2):
            assert R.parse_png(pngs[i][v])[2] == 2 and np.array_equal(R.decode_png(pngs[i][v]), want[i, v])


def test_record_round_trip(tmp_path):
    views = EC.mixed_batch(18, 16, 12).reshape(6, 3, 12, 16, 3)
    dev_pngs = R.encode_png_batch(torch.from_numpy(views.reshape(18, 12, 16, 3)).to(DEV))
    assert dev_pngs == R.encode_png_batch(views.reshape(18, 12, 16, 3))
    a, b = os.path.join(tmp_path, "device.record"), os.path.join(tmp_path, "host.record")
    R.write_tfrecords(a, [R.make_example(dev_pngs[3 * k:3 * k + 3], k) for k in range(6)])
    R.write_tfrecords(b, [R.make_example([R.encode_png(v) for v in views[k]], k) for k in range(6)])
    got = [(x.cpu().numpy(), y.numpy()) for x, y in R.ViewBatcher(a, 3, 8, 8, 2, "cuda:0", decode="host")]
    want = [(x.cpu().numpy(), y.numpy()) for x, y in R.ViewBatcher(b, 3, 8, 8, 2, "cuda:0", decode="host")]
    assert len(got) == len(want) == 3
    for (xa, ya), (xb, yb) in zip(got, want):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)


def test_non_default_stream():
    views = EC.mixed_batch(5, 100, 100)
    s = torch.cuda.Stream(device=DEV)
    assert s.cuda_stream != 0
    assert_same_as_host(views, EC.ADAPTIVE, EC.AUTO, device_encode(views, stream=s.cuda_stream))
