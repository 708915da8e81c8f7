"""Registration throughput on pairs of clouds sampled from a seeded mesh, one of each pair in a planted pose; prints one
JSON line.

    python tools/points_register_bench.py [--points 1000,10000,100000] [--iterations 30] [--steps 10] [--warmup 3] [--table]

N = 32 pairs of P points each: target m = sample_surface(mesh, P, seed m), source m = another sampling of the same mesh
(seed 1000 + m) turned 10 degrees about (1, 2, 3) and shifted by (0.03, -0.02, 0.05) of the unit sphere's radius.  The mesh
is an icosphere pulled out of round (scaled 1.0 x 0.7 x 0.45, with a bump), so the pose is observable.  Per size:
  - PointBatch.register(target, iterations) with tolerance 0 (device events around the whole call: the workspace and output
    allocations, the two grid builds, every round's launches, the read of the status words; after warm-up), with the
    source visited in cell order (the default) and in id order (gv_points_register_set_cell_order(0));
  - the same call with iterations = 1: the grid builds, one round and the outputs.  (ms - one_round_ms) / (iterations - 1)
    is then what a further round costs, as long as no pair stops early: `used` reports the rounds the pairs ran;
  - the pose error the call leaves (max |T T_planted - I|) and its rmse;
  - a torch restatement on the same device: per pair and round, chunked torch.cdist + argmin, centroids, a 3x3 covariance
    and torch.linalg.svd with the determinant fix, run for as many rounds as the slowest pair of the device call used.
    The route a user has without the kernels, not a bit-exact twin.  Above 20 000 points it runs on the first 2 pairs
    only and torch_ms is that time times N / 2 (torch_pairs says on how many it ran): the pairs are independent.
Which kernels the time goes to (grid build, nearest, sums, solve) is a profiler's question: run this tool with --points
10000 --steps 3 under a kernel trace.
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


def axis_angle(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def shape(R):
    """an icosphere out of round: three different half-axes and a bump on one side"""
    verts, tris = R.icosphere(4)
    v = verts.astype(np.float64) * np.array([1.0, 0.7, 0.45])
    v[:, 2] += 0.25 * np.exp(-8.0 * ((v[:, 0] - 0.4) ** 2 + (v[:, 1] - 0.2) ** 2))
    return v.astype(np.float32), tris


def torch_icp(src, tgt, N, P, rounds):
    """src, tgt [N * P, 3] fp32 on the device -> [N, 4, 4] fp64: cdist + argmin + SVD per pair and round."""
    out = []
    for m in range(N):
        p, y = src[m * P:(m + 1) * P].to(torch.float64), tgt[m * P:(m + 1) * P]
        Rm = torch.eye(3, dtype=torch.float64, device=src.device)
        t = torch.zeros(3, dtype=torch.float64, device=src.device)
        for _ in range(rounds):
            q = (p @ Rm.T + t).to(torch.float32)
            idx = torch.cat([torch.cdist(q[a:a + CHUNK], y).argmin(dim=1) for a in range(0, P, CHUNK)])
            ym = y[idx].to(torch.float64)
            cp, cy = p.mean(dim=0), ym.mean(dim=0)
            H = (p - cp).T @ (ym - cy)
            U, _, Vt = torch.linalg.svd(H)
            d = torch.sign(torch.linalg.det(Vt.T @ U.T))
            Rm = Vt.T @ torch.diag(torch.stack([torch.ones_like(d), torch.ones_like(d), d])) @ U.T
            t = cy - Rm @ cp
        T = torch.eye(4, dtype=torch.float64, device=src.device)
        T[:3, :3], T[:3, 3] = Rm, t
        out.append(T)
    return torch.stack(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000,10000,100000")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch restatement out (a profiler run)")
    ap.add_argument("--table", action="store_true", help="a plain-text table of the cases in front of the JSON line")
    a = ap.parse_args(argv)
    from gvcnn_tf_amd import _lib, render as R

    lib = _lib.load()
    dev = torch.device("cuda:0")
    N, it = a.n, a.iterations
    verts, tris = shape(R)
    planted = np.eye(4)
    planted[:3, :3], planted[:3, 3] = axis_angle((1, 2, 3), 10.0), (0.03, -0.02, 0.05)
    cases = []
    for P in [int(p) for p in a.points.split(",")]:
        target = R.PointBatch([R.sample_surface(verts, tris, P, seed=m)[0] for m in range(N)], dev)
        moved = [(R.sample_surface(verts, tris, P, seed=1000 + m)[0].astype(np.float64) @ planted[:3, :3].T
                  + planted[:3, 3]).astype(np.float32) for m in range(N)]
        source = R.PointBatch(moved, dev)
        row = {"points": P, "N": N, "iterations": it}
        row["ms"] = round(timed(lambda: source.register(target, it), a.steps, a.warmup), 4)
        lib.gv_points_register_set_cell_order(0)
        try:
            row["id_order_ms"] = round(timed(lambda: source.register(target, it), a.steps, a.warmup), 4)
        finally:
            lib.gv_points_register_set_cell_order(1)
        row["one_round_ms"] = round(timed(lambda: source.register(target, 1), a.steps, a.warmup), 4)
        row["further_round_ms"] = round((row["ms"] - row["one_round_ms"]) / max(it - 1, 1), 4)
        new, transforms, (rmse, inliers, used) = source.register(target, it, return_info=True)
        T = transforms.cpu().numpy()
        used = used.cpu().numpy()
        row["used"] = [int(used.min()), int(used.max())]
        row["pose_error"] = float("%.3g" % np.abs(T @ planted - np.eye(4)).max())
        row["rmse"] = float("%.3g" % rmse.cpu().numpy().max())
        row["status"] = sorted(set(new.register_status.tolist()))
        if not a.no_torch:
            rounds = int(used.max())
            few, tp = (max(a.steps // 4, 2), N) if P <= 20000 else (1, min(N, 2))
            row["torch_rounds"], row["torch_pairs"] = rounds, tp
            ms = timed(lambda: torch_icp(source.points, target.points, tp, P, rounds), few, 1)
            row["torch_ms"] = round(ms * N / tp, 4)
            Tt = torch_icp(source.points, target.points, tp, P, rounds).cpu().numpy()
            row["torch_pose_error"] = float("%.3g" % np.abs(Tt @ planted - np.eye(4)).max())
        cases.append(row)
        del source, target, new
        torch.cuda.empty_cache()
    if a.table:
        print("%8s %11s %12s %13s %17s %9s %11s %10s" % ("points", "register ms", "id order ms", "one round ms",
                                                         "further round ms", "used", "pose error", "torch ms"))
        for c in cases:
            print("%8d %11.3f %12.3f %13.3f %17.4f %9s %11.3g %10s" % (
                c["points"], c["ms"], c["id_order_ms"], c["one_round_ms"], c["further_round_ms"],
                "%d-%d" % tuple(c["used"]), c["pose_error"], "%.3f" % c["torch_ms"] if "torch_ms" in c else "-"))
    print(json.dumps({"metric": "points_register_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
