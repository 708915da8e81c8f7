"""Rasteriser throughput on seeded synthetic meshes; prints one JSON line.

    python tools/render_bench.py [--forward c4|c2] [--steps 20] [--warmup 5]

Cases: icospheres of 80, 1 280, 20 480 and 327 680 faces and a giant/tiny mix (two screen-size triangles + 20 000
small ones), N = 32 meshes x V = 12 views at 224^2 and 299^2, each mesh under its own random rotation.  Per case: ms per
batch (device events around the whole render: prepare, the one host read of the tile-list size, draw; after warm-up),
meshes/s, views/s and triangle-views/s.  --forward c4 (bf16 ResNet-v2-50) or c2 (fp32 Inception-v3): the GVCNN
forward time of the same views, so the render cost reads against what it feeds.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", choices=sorted(FORWARD))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--sizes", default="224,299")
    a = ap.parse_args(argv)
    import gvcnn_tf_amd as gv
    from gvcnn_tf_amd import render as R

    dev = torch.device("cuda:0")
    N, V = a.n, a.views
    meshes = {"ico80": R.icosphere(1), "ico1k": R.icosphere(3), "ico20k": R.icosphere(5), "ico330k": R.icosphere(7),
              "giant_tiny": giant_tiny()}
    rots = R.random_rotations(N, "so3", seed=0)
    cases = []
    for size in [int(s) for s in a.sizes.split(",")]:
        r = R.ViewRenderer(V, size, size, device=dev)
        out = torch.empty((N, V, size, size, 3), dtype=torch.float32, device=dev)
        for name, m in meshes.items():
            batch = R.MeshBatch([m] * N, dev)
            ms = timed(lambda: r.render(batch, rotations=rots, out=out), a.steps, a.warmup)
            case = {"mesh": name, "faces": int(len(m[1])), "size": size, "N": N, "V": V, "ms": round(ms, 4),
                    "meshes_per_s": round(N / ms * 1e3, 1), "views_per_s": round(N * V / ms * 1e3, 1),
                    "tri_views_per_s": float("%.4g" % (N * V * len(m[1]) / ms * 1e3))}
            cases.append(case)
            del batch
        if a.forward:
            backbone, storage = FORWARD[a.forward]
            eng = gv.GVCNN(backbone, N, V, size, size, 40, 10, device=dev, storage=storage)
            ms = timed(lambda: eng.forward(out, check=False), a.steps, a.warmup)
            cases.append({"forward": a.forward, "backbone": backbone, "storage": storage, "size": size, "N": N, "V": V,
                          "ms": round(ms, 4), "views_per_s": round(N * V / ms * 1e3, 1)})
            del eng
            torch.cuda.empty_cache()
    print(json.dumps({"metric": "render_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
