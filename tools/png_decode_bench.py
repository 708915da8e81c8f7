#!/usr/bin/env python3
"""What does the device PNG decode cost, and what must it sustain?  On 384 views of tools/pipeline_bench.py's synthetic
set (256x256, Pillow, adaptive filters):
  1. gv_png_decode_batch alone: device events around warmed-up launches over a window of at least a second
     (ms per batch, views/s), and gv_preprocess_views (256 -> 224) on the decoded batch beside it for scale;
  2. the rate the stage is fed at: ViewBatcher(decode="device") with the device work of a batch stubbed out — GZIP
     reader threads + parse_example + parse_png + shuffle-free batching — at 1 and 4 record files.
    python tools/png_decode_bench.py [--views 384] [--shapes 768] [--files 1 4]"""
import argparse
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pipeline_bench import render  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=384)
    ap.add_argument("--shapes", type=int, default=768)
    ap.add_argument("--files", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    import gvcnn_tf_amd                              # noqa: F401
    from gvcnn_tf_amd import _lib, records as R
    from gvcnn_tf_amd.model import _st
    from PIL import Image
    rng = np.random.RandomState(0)
    encoded = []
    for _ in range(24):
        buf = io.BytesIO()
        Image.fromarray(render(rng), "RGB").save(buf, format="PNG")
        encoded.append(buf.getvalue())
    lib, dev = _lib.load(), torch.device("cuda:0")
    pngs = [R.parse_png(encoded[i % len(encoded)]) for i in range(a.views)]
    buf, images, (h0, w0) = R.pack_png_batch(pngs)
    n = len(pngs)
    streams = torch.from_numpy(buf).to(dev)
    out = torch.empty((n, h0, w0, 3), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = lib.gv_png_decode_workspace_bytes(n, h0 * (1 + 4 * w0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty((n, 224, 224, 3), dtype=torch.float32, device=dev)

    def decode():
        _lib.check(lib.gv_png_decode_batch(streams.data_ptr(), buf.size, images, n, h0, w0, streams.data_ptr(), out.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), ws_bytes, _st()), "gv_png_decode_batch")

    def preprocess():
        _lib.check(lib.gv_preprocess_views(out.data_ptr(), n, h0, w0, 224, 224, None, None, dst.data_ptr(), _st()),
                   "gv_preprocess_views")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps, ms = 4, 0.0
        while True:                                              # grow the window until it spans a.seconds
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 1e3 * a.seconds:
                return ms / reps, reps
            reps = max(reps * 2, int(reps * 1.2e3 * a.seconds / max(ms, 1e-3)))
    print("%d views %dx%d, %.1f KB of zlib stream per view, %.2f MB per batch (decoded: %.1f MB)"
          % (n, h0, w0, sum(len(p[4]) for p in pngs) / n / 1e3, buf.size / 1e6, out.numel() / 1e6))
    ms, reps = timed(decode)
    assert not status.cpu().numpy().any()
    want = np.stack([R.decode_png(e) for e in encoded])
    assert np.array_equal(out.cpu().numpy()[:len(encoded)], want[:n])
    print("gv_png_decode_batch:  %8.3f ms per batch  %9.0f views/s  (%d launches in one window)" % (ms, n / ms * 1e3, reps))
    ms, reps = timed(preprocess)
    print("gv_preprocess_views:  %8.3f ms per batch  %9.0f views/s  (%d launches in one window)" % (ms, n / ms * 1e3, reps))

    tmp = tempfile.mkdtemp(prefix="gv_pngb_")
    V = 12
    recs = [R.make_example([encoded[(s * V + v) % len(encoded)] for v in range(V)], s % 40) for s in range(a.shapes)]
    for nf in [f for f in a.files if f > 0]:                    # (--files 0: the kernels only)
        paths = [os.path.join(tmp, "s_%d_of_%d.record" % (f, nf)) for f in range(nf)]
        for f, p in enumerate(paths):
            R.write_tfrecords(p, recs[f::nf])
        for _ in range(3):
            vb = R.ViewBatcher(paths if nf > 1 else paths[0], V, 224, 224, 32, "cuda:0", workers=1, decode="device")
            vb._batch_device = lambda items, labels: (None, None)        # the kernels (and the packing) out of the timing
            t0, k = time.time(), 0
            for _ in vb:
                k += 32 * V
            dt = time.time() - t0
            vb.close()
            print("feed, %d file(s): GZIP reader threads + parse (no device work): %8.0f views/s  (%d views in %.2f s)"
                  % (nf, k / dt, k, dt))


if __name__ == "__main__":
    main()
