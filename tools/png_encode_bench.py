#!/usr/bin/env python3
"""What does the device PNG encode cost next to the render that feeds it and to the host path it replaces?  On 384 views
(32 meshes x 12 views, 224 x 224) of render.icosphere(2) under random rotations, rendered on the device:
  1. gv_png_encode_batch (adaptive filter, colour auto) between device events: warmed-up launches over a window of at
     least a second; the render of the same batch beside it (whole render_uint8, and its gv_render_draw calls alone);
  2. the host path on the same box: .cpu() of the 58 MB of pixels, then records.encode_png per view (zlib level 6, one
     core), wall clock, --host-repeats times;
  3. the bytes of both encodings of the batch (whole PNG files), and a decode of every device-encoded view.
--surface gray renders a gray surface (colour type 0) instead of the renderer's default colour (colour type 2).
Appends the lines it prints to --out as well (with the command in front).
    python tools/png_encode_bench.py [--meshes 32] [--views 12] [--size 224] [--out profiles/png_encode_bench.txt]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from render_bench import timed_split  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--surface", default="default", choices=("default", "gray"),
                    help="default: the renderer's default surface colour (not gray: colour type 2, what "
                         "tools/render_modelnet.py writes); gray: a gray surface (colour type 0)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import gvcnn_tf_amd                              # noqa: F401
    from gvcnn_tf_amd import _lib, records as R, render
    from gvcnn_tf_amd.model import _st
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    lib, dev = _lib.load(), torch.device("cuda:0")
    r = render.ViewRenderer(a.views, a.size, a.size, device=dev, **({"color": (0.6, 0.6, 0.6)} if a.surface == "gray" else {}))
    batch = render.MeshBatch([render.icosphere(2)] * a.meshes, dev)
    rot = render.random_rotations(a.meshes, mode="z", seed=0)
    views = r.render_uint8(batch, rot)
    n, h, w = a.meshes * a.views, a.size, a.size
    src = views.view(n, h, w, 3)
    stride = lib.gv_png_encode_bound(h, w)
    ws_bytes = lib.gv_png_encode_workspace_bytes(n, h, w)
    out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    info = torch.empty((2, n), dtype=torch.int32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def encode():
        _lib.check(lib.gv_png_encode_batch(src.data_ptr(), n, h, w, _lib.GV_PNG_FILTER_ADAPTIVE, _lib.GV_PNG_COLOR_AUTO,
                                           out.data_ptr(), stride, info[0].data_ptr(), info[1].data_ptr(), ws.data_ptr(), ws_bytes,
                                           _st()), "gv_png_encode_batch")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps = 4
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
    say("%d views %dx%d of icosphere(2), %s surface: %.1f MB of pixels, workspace %.1f MB, stream slots %.1f MB"
        % (n, h, w, a.surface, src.numel() / 1e6, ws_bytes / 1e6, out.numel() / 1e6))
    ms, reps = timed(encode)
    say("gv_png_encode_batch:      %9.3f ms per batch  %9.0f views/s  (%d launches in one window)" % (ms, n / ms * 1e3, reps))
    rms, pms, dms, _ = timed_split(r, lambda: r.render_uint8(batch, rot, out=views), 20, 5)
    say("render_uint8 (whole):     %9.3f ms per batch; its gv_render_prepare %.3f ms, gv_render_draw %.3f ms (device events)"
        % (rms, pms, dms))
    say("gv_png_decode_batch (profiles/png_decode_bench.txt, 384 views 256x256, for scale): 10.498 ms per batch")
    host_ms = []
    for _ in range(a.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pix = views.cpu().numpy()
        t1 = time.perf_counter()
        host_pngs = [R.encode_png(pix[i, v]) for i in range(a.meshes) for v in range(a.views)]
        t2 = time.perf_counter()
        host_ms.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    for c, e in host_ms:
        say("host path (.cpu() + encode_png loop): %9.1f ms copy + %9.1f ms zlib level 6 on one core = %9.1f ms per batch"
            % (c, e, c + e))
    t0 = time.perf_counter()
    dev_pngs = R.encode_png_batch(src)
    t1 = time.perf_counter()
    say("records.encode_png_batch (device encode + copy of the used stream bytes + chunk framing, wall clock): %.1f ms"
        % (1e3 * (t1 - t0)))
    length, ctype = info.cpu().numpy()
    assert set(ctype.tolist()) == ({0} if a.surface == "gray" else {2}), ctype
    pix = views.cpu().numpy().reshape(n, h, w, 3)
    for i in range(n):
        assert np.array_equal(R.decode_png(dev_pngs[i]), pix[i]), i
    say("bytes of the batch: device encoder %d (%.2f KB per view, colour type %d, adaptive filter), encode_png %d (%.2f KB per "
        "view, RGB, filter 0, zlib level 6); every device-encoded view decodes to its pixels"
        % (sum(map(len, dev_pngs)), sum(map(len, dev_pngs)) / n / 1e3, int(ctype[0]), sum(map(len, host_pngs)), sum(map(len, host_pngs)) / n / 1e3))
    if a.out:
        with open(a.out, "a") as f:
            f.write("python tools/png_encode_bench.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
