"""Normal estimation throughput on clouds sampled from a seeded mesh; prints one JSON line.

    python tools/point_normals_bench.py [--points 1000,10000,100000] [--k 16] [--steps 10] [--warmup 3] [--table]

N = 32 clouds of P points each from sample_surface(icosphere(5)) (one seed per cloud), k = 16, orient "outward".  Per size:
  - PointBatch.estimate_normals (device events around the whole call: the workspace and output allocations, the launches,
    the read of the status words; after warm-up);
  - a torch restatement of the same job on the same device: per cloud, chunked torch.cdist + topk(k, largest=False), the
    neighbourhoods gathered, a batched covariance in fp64 and torch.linalg.eigh, the sign from the bounding box's centre.
    cdist's own fp32 and eigh's own solver: the route a user has without the kernels, not a bit-exact twin;
  - render_points(shading="normal") alone on the estimated batch (12 views at 224^2, radius "auto").
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from render_bench import timed  # noqa: E402

CHUNK = 4096                                                        # query rows per cdist block


def torch_normals(pts, N, P, k, out):
    """pts [N * P, 3] fp32 on the device -> out, normals [N * P, 3] fp32: cdist + topk + covariance + eigh per cloud."""
    for m in range(N):
        p = pts[m * P:(m + 1) * P]
        idx = torch.cat([torch.cdist(p[a:a + CHUNK], p).topk(min(k, P), dim=1, largest=False).indices
                         for a in range(0, P, CHUNK)])
        nb = p[idx].to(torch.float64)                                   # [P, k, 3]
        e = nb - nb.mean(dim=1, keepdim=True)
        cov = e.transpose(1, 2) @ e
        n = torch.linalg.eigh(cov).eigenvectors[:, :, 0]
        c = (p.amin(0) + p.amax(0)).to(torch.float64) * 0.5
        flip = (n * (p.to(torch.float64) - c)).sum(1) < 0
        out[m * P:(m + 1) * P] = torch.where(flip[:, None], -n, n).to(torch.float32)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000,10000,100000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--table", action="store_true", help="a plain-text table of the cases in front of the JSON line")
    a = ap.parse_args(argv)
    from gvcnn_tf_amd import render as R

    dev = torch.device("cuda:0")
    N, V, S, k = a.n, a.views, a.size, a.k
    verts, tris = R.icosphere(5)
    r = R.ViewRenderer(V, S, S, device=dev, point_reflection=dict(light="camera", two_sided=True))
    out = torch.empty((N, V, S, S, 3), dtype=torch.float32, device=dev)
    cases = []
    for P in [int(p) for p in a.points.split(",")]:
        batch = R.PointBatch([R.sample_surface(verts, tris, P, seed=1 + m)[0] for m in range(N)], dev)
        row = {"points": P, "N": N, "k": k}
        row["estimate_ms"] = round(timed(lambda: batch.estimate_normals(k), a.steps, a.warmup), 4)
        row["points_per_s"] = float("%.4g" % (N * P / row["estimate_ms"] * 1e3))
        row["status"] = sorted(set(batch.normal_status.tolist()))
        theirs = torch.empty_like(batch.points)
        row["torch_ms"] = round(timed(lambda: torch_normals(batch.points, N, P, k, theirs), max(a.steps // 4, 2), 1), 4)
        # how far the two routes agree, for the record: the angle between their (oriented) normals
        cosine = (theirs * batch.normals).sum(1).clamp(-1, 1)
        row["torch_agree_deg_p99"] = round(float(torch.rad2deg(torch.acos(cosine)).quantile(0.99)), 4)
        row["render_normal_ms"] = round(timed(lambda: r.render_points(batch, out=out, shading="normal"), a.steps, a.warmup), 4)
        cases.append(row)
        del batch
        torch.cuda.empty_cache()
    if a.table:
        print("%8s %12s %12s %10s %17s" % ("points", "estimate ms", "Mpoints/s", "torch ms", "render normal ms"))
        for c in cases:
            print("%8d %12.3f %12.2f %10.3f %17.3f" % (c["points"], c["estimate_ms"], c["points_per_s"] / 1e6, c["torch_ms"],
                                                      c["render_normal_ms"]))
    print(json.dumps({"metric": "point_normals_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
