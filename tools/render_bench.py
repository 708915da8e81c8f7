"""Rasteriser throughput on seeded synthetic meshes; prints one JSON line.

    python tools/render_bench.py [--forward c4|c2] [--samples 1,2,4] [--pool-baseline] [--steps 20] [--warmup 5]
                                 [--shading smooth [--light camera] [--diffuse lambert] [--specular 0.3]]

Cases: icospheres of 80, 1 280, 20 480 and 327 680 faces and a giant/tiny mix (two screen-size triangles + 20 000
small ones), N = 32 meshes x V = 12 views at 224^2 and 299^2, each mesh under its own random rotation.  Per case: ms per
batch (device events around the whole render: prepare, the one host read of the tile-list size, draw; after warm-up),
meshes/s, views/s and triangle-views/s.  --forward c4 (bf16 ResNet-v2-50) or c2 (fp32 Inception-v3): the GVCNN
forward time of the same views, so the render cost reads against what it feeds.  --samples: the anti-aliased renders
(S x S samples per pixel resolved in the rasteriser), one case per S, each with the device time of its prepare and draw
calls (events around the two C-ABI calls; the rest of "ms" is the host read between them).  --pool-baseline: next to
every S = 2 case whose doubled side the rasteriser takes (<= 512), what one sample per pixel can do: render at 2H x 2W
and average-pool in torch.  --shading smooth: the same cases with interpolated vertex normals (gv_render_vertex_normals +
gv_render_draw_smooth); the normals kernel's own device time is reported next to prepare and draw.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FORWARD = {"c4": ("resnet_v2_50", "bf16"), "c2": ("inception_v3", "f32")}


def giant_tiny(n=20000, seed=0):
    rng = np.random.RandomState(seed)
    qv = np.array([[0, -1, -1], [0, 1, -1], [0, 1, 1], [0, -1, 1]], np.float64)
    c = rng.uniform(-0.6, 0.6, size=(n, 1, 3))
    small = (c + rng.uniform(-0.01, 0.01, size=(n, 3, 3))).reshape(-1, 3)
    v = np.concatenate([qv, small]).astype(np.float32)
    t = np.concatenate([[[0, 1, 2], [0, 2, 3]], 4 + np.arange(3 * n).reshape(n, 3)]).astype(np.int32)
    return v, t


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


class SplitTimer:
    """Stands in for the library of a ViewRenderer: device events around every prepare and every draw call."""

    def __init__(self, lib):
        self.lib, self.events = lib, {"prepare": [], "draw": [], "normals": []}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        kind = ("prepare" if name.startswith("gv_render_prepare") else "draw" if name.startswith("gv_render_draw") else
                "normals" if name == "gv_render_vertex_normals" else None)
        if kind is None:
            return fn

        def call(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.events[kind].append((a, b))
            return rc
        return call

    def ms(self, kind, steps):
        """device ms per render of the calls of `kind` (after a synchronize)."""
        return sum(a.elapsed_time(b) for a, b in self.events[kind]) / steps


def timed_split(r, fn, steps, warmup):
    """(ms, prepare ms, draw ms, normals ms) per render: the whole render as `timed` measures it, then the calls' own
    times in a second pass (the extra events stay out of the first).  normals ms is 0 for a flat renderer."""
    ms = timed(fn, steps, warmup)
    lib = r.lib
    r.lib = t = SplitTimer(lib)
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    finally:
        r.lib = lib
    return ms, t.ms("prepare", steps), t.ms("draw", steps), t.ms("normals", steps)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", choices=sorted(FORWARD))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--sizes", default="224,299")
    ap.add_argument("--samples", default="1", help="samples per pixel and axis, comma separated (1, 2, 4)")
    ap.add_argument("--pool-baseline", action="store_true",
                    help="next to S = 2: one sample per pixel at twice the side, then avg_pool2d")
    ap.add_argument("--shading", default="flat", choices=("flat", "smooth"))
    ap.add_argument("--light", default="world", choices=("world", "camera"), help="camera: a headlight (smooth only)")
    ap.add_argument("--diffuse", default="wrap", choices=("wrap", "lambert"))
    ap.add_argument("--specular", type=float, default=0.0)
    ap.add_argument("--shininess", type=int, default=16, help="exponent of the highlight: 1, 2, 4, ..., 128")
    ap.add_argument("--two-sided", action="store_true", help="shade both faces alike (one normal table per view)")
    ap.add_argument("--meshes", default="", help="comma separated subset of the mesh names (default: all)")
    ap.add_argument("--table", action="store_true", help="a plain-text table of the cases in front of the JSON line")
    a = ap.parse_args(argv)
    import gvcnn_tf_amd as gv
    from gvcnn_tf_amd import render as R

    dev = torch.device("cuda:0")
    N, V = a.n, a.views
    meshes = {"ico80": R.icosphere(1), "ico1k": R.icosphere(3), "ico20k": R.icosphere(5), "ico330k": R.icosphere(7),
              "giant_tiny": giant_tiny()}
    if a.meshes:
        meshes = {k: meshes[k] for k in a.meshes.split(",")}
    rots = R.random_rotations(N, "so3", seed=0)
    samples = [int(s) for s in a.samples.split(",")]
    cases = []
    for size in [int(s) for s in a.sizes.split(",")]:
        out = torch.empty((N, V, size, size, 3), dtype=torch.float32, device=dev)
        for S in samples:
            r = R.ViewRenderer(V, size, size, device=dev, samples=S, shading=a.shading, diffuse=a.diffuse,
                               specular=a.specular, shininess=a.shininess, two_sided=a.two_sided,
                               **({"light": "camera"} if a.light == "camera" else {}))
            for name, m in meshes.items():
                batch = R.MeshBatch([m] * N, dev)
                ms, prep, draw, nrm = timed_split(r, lambda: r.render(batch, rotations=rots, out=out), a.steps,
                                                  a.warmup)
                case = {"mesh": name, "faces": int(len(m[1])), "size": size, "samples": S, "N": N, "V": V,
                        "shading": a.shading, "ms": round(ms, 4), "prepare_ms": round(prep, 4),
                        "draw_ms": round(draw, 4), "normals_ms": round(nrm, 4),
                        "meshes_per_s": round(N / ms * 1e3, 1), "views_per_s": round(N * V / ms * 1e3, 1),
                        "tri_views_per_s": float("%.4g" % (N * V * len(m[1]) / ms * 1e3))}
                cases.append(case)
                if a.pool_baseline and S == 2 and 2 * size <= R.MAX_SIDE:
                    big = R.ViewRenderer(V, 2 * size, 2 * size, device=dev)
                    wide = torch.empty((N, V, 2 * size, 2 * size, 3), dtype=torch.float32, device=dev)

                    def pooled():
                        big.render(batch, rotations=rots, out=wide, quantize=False)
                        x = wide.view(N * V, 2 * size, 2 * size, 3).permute(0, 3, 1, 2)       # NCHW view of NHWC
                        y = torch.nn.functional.avg_pool2d(x, 2)
                        out.view(N * V, size, size, 3).copy_(y.permute(0, 2, 3, 1))
                    ms = timed(pooled, a.steps, a.warmup)
                    cases.append({"mesh": name, "faces": int(len(m[1])), "size": size, "samples": 1,
                                  "baseline": "render at %d^2 + avg_pool2d(2)" % (2 * size), "N": N, "V": V,
                                  "ms": round(ms, 4), "meshes_per_s": round(N / ms * 1e3, 1),
                                  "views_per_s": round(N * V / ms * 1e3, 1)})
                    del big, wide
                del batch
        if a.forward:
            backbone, storage = FORWARD[a.forward]
            eng = gv.GVCNN(backbone, N, V, size, size, 40, 10, device=dev, storage=storage)
            ms = timed(lambda: eng.forward(out, check=False), a.steps, a.warmup)
            cases.append({"forward": a.forward, "backbone": backbone, "storage": storage, "size": size, "N": N, "V": V,
                          "ms": round(ms, 4), "views_per_s": round(N * V / ms * 1e3, 1)})
            del eng
            torch.cuda.empty_cache()
    if a.table:
        print("%-11s %7s %5s %2s  %9s %10s %9s %10s  %s" % ("mesh", "faces", "size", "S", "ms/batch", "prepare ms", "draw ms",
                                                            "normals ms", ""))
        for c in cases:
            if "mesh" in c:
                print("%-11s %7d %5d %2d  %9.3f %10s %9s %10s  %s" % (
                    c["mesh"], c["faces"], c["size"], c["samples"], c["ms"],
                    "%.3f" % c["prepare_ms"] if "prepare_ms" in c else "-",
                    "%.3f" % c["draw_ms"] if "draw_ms" in c else "-",
                    "%.3f" % c["normals_ms"] if c.get("shading") == "smooth" else "-", c.get("baseline", "")))
    print(json.dumps({"metric": "render_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
