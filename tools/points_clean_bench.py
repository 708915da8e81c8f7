"""Cleaning throughput on clouds sampled from a seeded mesh with planted outliers; prints one JSON line.

    python tools/points_clean_bench.py [--points 1000,10000,100000] [--k 16] [--steps 10] [--warmup 3] [--table]

N = 32 clouds of P points each: 99 % from sample_surface(icosphere(5)) (one seed per cloud), 1 % planted at 4 to 8 radii in
random directions.  Per size:
  - PointBatch.remove_outliers(k, 2.0) and PointBatch.voxel_downsample(0.02, relative=True) (device events around the
    whole call: the workspace and output allocations, the launches, the read of the counts and status words; after
    warm-up);
  - remove_outliers on what voxel_downsample returned (the usual order: downsample first);
  - PointBatch.estimate_normals(k) on the batch as it came and on the batch remove_outliers returned: what the far
    points cost the search grid;
  - a torch restatement of the two jobs on the same device: per cloud, chunked torch.cdist + topk(k + 1, largest=False)
    without the self column, mean / std and a mask; and torch.unique(dim=0, return_inverse=True) on the integer cells +
    index_add_ for the centroids.  The route a user has without the kernels, not a bit-exact twin.
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

from render_bench import timed  # noqa: E402

CHUNK = 4096                                                        # query rows per cdist block


def dirty_cloud(R, verts, tris, P, seed):
    """P points: all but P // 100 on the unit icosphere, the rest at 4 to 8 radii"""
    n_out = P // 100
    rng = np.random.RandomState(1000 + seed)
    d = rng.normal(size=(n_out, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4.0, 8.0, size=(n_out, 1))
    return np.concatenate([R.sample_surface(verts, tris, P - n_out, seed=seed)[0], far.astype(np.float32)])


def torch_outliers(pts, N, P, k, ratio):
    """pts [N * P, 3] fp32 on the device -> the kept points of every cloud: cdist + topk + mean / std + mask."""
    out = []
    for m in range(N):
        p = pts[m * P:(m + 1) * P]
        d = torch.cat([torch.cdist(p[a:a + CHUNK], p).topk(min(k + 1, P), dim=1, largest=False).values[:, 1:]
                       for a in range(0, P, CHUNK)])
        mean = d.to(torch.float64).mean(dim=1)
        out.append(p[mean <= mean.mean() + ratio * mean.std()])
    return out


def torch_voxels(pts, N, P, voxel):
    """pts [N * P, 3] fp32 on the device -> the voxel centroids of every cloud: unique rows + index_add_."""
    out = []
    for m in range(N):
        p = pts[m * P:(m + 1) * P]
        mn = p.amin(0)
        h = voxel * (p.amax(0) - mn).max()
        cells = ((p - mn) / h).to(torch.int64)
        uniq, inv = torch.unique(cells, dim=0, return_inverse=True)
        sums = torch.zeros((len(uniq), 3), dtype=torch.float64, device=p.device).index_add_(0, inv, p.to(torch.float64))
        cnt = torch.bincount(inv, minlength=len(uniq)).to(torch.float64)
        out.append((sums / cnt[:, None]).to(torch.float32))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000,10000,100000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--table", action="store_true", help="a plain-text table of the cases in front of the JSON line")
    a = ap.parse_args(argv)
    from gvcnn_tf_amd import render as R

    dev = torch.device("cuda:0")
    N, k = a.n, a.k
    verts, tris = R.icosphere(5)
    cases = []
    for P in [int(p) for p in a.points.split(",")]:
        batch = R.PointBatch([dirty_cloud(R, verts, tris, P, 1 + m) for m in range(N)], dev)
        row = {"points": P, "N": N, "k": k, "planted": N * (P // 100)}
        row["remove_ms"] = round(timed(lambda: batch.remove_outliers(k, a.ratio), a.steps, a.warmup), 4)
        row["voxel_ms"] = round(timed(lambda: batch.voxel_downsample(a.voxel, relative=True), a.steps, a.warmup), 4)
        clean, index = batch.remove_outliers(k, a.ratio, return_index=True)
        kept = int(clean.point_offsets_host[-1])
        ids = index[:kept].cpu().numpy()
        inlier = P - P // 100                                       # ids below it are surface points
        row["kept"] = kept
        row["planted_kept"] = int((ids >= inlier).sum())
        row["voxels"] = int(batch.voxel_downsample(a.voxel, relative=True).point_offsets_host[-1])
        row["status"] = sorted(set(clean.clean_status.tolist()))
        small = batch.voxel_downsample(a.voxel, relative=True)      # the usual order: downsample first
        row["remove_after_voxel_ms"] = round(timed(lambda: small.remove_outliers(k, a.ratio), a.steps, a.warmup), 4)
        row["kept_after_voxel"] = int(small.remove_outliers(k, a.ratio).point_offsets_host[-1])
        row["normals_before_ms"] = round(timed(lambda: batch.estimate_normals(k), a.steps, a.warmup), 4)
        row["normals_after_ms"] = round(timed(lambda: clean.estimate_normals(k), a.steps, a.warmup), 4)
        few = max(a.steps // 4, 2)
        row["torch_remove_ms"] = round(timed(lambda: torch_outliers(batch.points, N, P, k, a.ratio), few, 1), 4)
        row["torch_voxel_ms"] = round(timed(lambda: torch_voxels(batch.points, N, P, a.voxel), few, 1), 4)
        row["torch_kept"] = int(sum(len(c) for c in torch_outliers(batch.points, N, P, k, a.ratio)))
        row["torch_voxels"] = int(sum(len(c) for c in torch_voxels(batch.points, N, P, a.voxel)))
        cases.append(row)
        del batch, clean
        torch.cuda.empty_cache()
    if a.table:
        print("%8s %10s %9s %19s %15s %14s %13s %12s" % ("points", "remove ms", "voxel ms", "remove after voxel",
                                                         "normals before", "normals after", "torch remove", "torch voxel"))
        for c in cases:
            print("%8d %10.3f %9.3f %19.3f %15.3f %14.3f %13.3f %12.3f" % (
                c["points"], c["remove_ms"], c["voxel_ms"], c["remove_after_voxel_ms"], c["normals_before_ms"],
                c["normals_after_ms"], c["torch_remove_ms"], c["torch_voxel_ms"]))
    print(json.dumps({"metric": "points_clean_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
