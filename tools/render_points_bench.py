"""Point splatter throughput on clouds sampled from a seeded mesh; prints one JSON line.

    python tools/render_points_bench.py [--points 1000,10000,100000] [--steps 20] [--warmup 5] [--table]

N = 32 clouds x V = 12 views at 224^2, each cloud under its own random rotation, radius "auto".  Per cloud size:
  - render_points, shading "depth" and "normal" (device events around the whole call: prepare, the one host read of the
    tile-list size, draw; after warm-up);
  - a torch restatement of the same job: normalise, rotate, project, then a square splat of the auto radius with
    scatter_reduce_(amin) on int64 keys (depth << 32 | id), one scatter per pixel offset of the square, and the depth
    shading from the winning keys.  fp32 with torch's own fusing, squares for discs: it is the route a user has without
    the kernels, not a bit-exact twin;
  - for scale, render() of the mesh the clouds were sampled from (icosphere(5), 20 480 faces).
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


def torch_splat(r, pts, offsets, rots, radius_px, out):
    """pts [sum P, 3] and int64 offsets [N + 1] on the device (equal sizes P), rots [N, 3, 3]: square splats through
    scatter_reduce_(amin); writes out [N, V, H, W, 3] (depth shading, quantised like the renderer's default)."""
    d = r.desc
    N, V, H, W = len(offsets) - 1, r.V, r.H, r.W
    P = pts.shape[0] // N
    p = pts.view(N, P, 3)
    c = (p.amin(1, keepdim=True) + p.amax(1, keepdim=True)) * 0.5
    q = p - c
    scale = d.fit / q.square().sum(2).amax(1).sqrt()
    w = torch.einsum("nij,npj->npi", rots, q * scale[:, None, None])
    cam = torch.einsum("vij,npj->nvpi", r.cameras, w)                     # [N, V, P, 3]
    sx = W * 0.5 + cam[..., 0] * d.proj_scale
    sy = H * 0.5 - cam[..., 1] * d.proj_scale
    Z = ((cam[..., 2] + 1.0) * 0.5).clamp(0, 1).mul(16777215.0).round().to(torch.int64)
    ids = torch.arange(P, device=pts.device, dtype=torch.int64).view(1, 1, P)
    key = (Z << 32) | ids
    ix, iy = sx.floor().to(torch.int64), sy.floor().to(torch.int64)
    base = (torch.arange(N * V, device=pts.device, dtype=torch.int64) * (H * W)).view(N, V, 1)
    best = torch.full((N * V * H * W,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=pts.device)
    for dy in range(-radius_px, radius_px + 1):
        for dx in range(-radius_px, radius_px + 1):
            x, y = ix + dx, iy + dy
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            idx = (base + y.clamp(0, H - 1) * W + x.clamp(0, W - 1))[ok]
            best.scatter_reduce_(0, idx, key[ok], "amin")
    hit = best != torch.iinfo(torch.int64).max
    t = (best >> 32).to(torch.float32) / 16777215.0
    f = d.ambient + (1.0 - d.ambient) * (1.0 - t)
    color = torch.tensor(list(d.color), device=pts.device)
    bg = torch.tensor(list(d.background), device=pts.device)
    col = torch.where(hit[:, None], color[None, :] * f[:, None], bg[None, :])
    u8 = (col * 255.0 + 0.5).floor().clamp(0, 255)
    out.view(-1, 3).copy_(u8 / 255.0 - 0.5)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000,10000,100000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--table", action="store_true", help="a plain-text table of the cases in front of the JSON line")
    a = ap.parse_args(argv)
    from gvcnn_tf_amd import render as R

    dev = torch.device("cuda:0")
    N, V, S = a.n, a.views, a.size
    verts, tris = R.icosphere(5)
    rots = R.random_rotations(N, "so3", seed=0)
    rots_dev = torch.from_numpy(rots).to(dev)
    r = R.ViewRenderer(V, S, S, device=dev, point_reflection=dict(light="camera", diffuse="lambert"))
    out = torch.empty((N, V, S, S, 3), dtype=torch.float32, device=dev)
    cases = []
    for P in [int(p) for p in a.points.split(",")]:
        cloud = R.sample_surface(verts, tris, P, seed=1)
        batch = R.PointBatch([cloud] * N, dev)
        radius = R.auto_point_radius(P, r.desc.fit, r.desc.proj_scale)
        px = int(np.ceil(float(radius) * r.desc.proj_scale - 0.5))          # the square that holds the disc's pixels
        row = {"points": P, "size": S, "N": N, "V": V, "radius_px": round(float(radius) * r.desc.proj_scale, 3)}
        for shading in ("depth", "normal"):
            ms = timed(lambda: r.render_points(batch, rotations=rots, out=out, shading=shading), a.steps, a.warmup)
            row["%s_ms" % shading] = round(ms, 4)
        row["point_views_per_s"] = float("%.4g" % (N * V * P / row["depth_ms"] * 1e3))
        ms = timed(lambda: torch_splat(r, batch.points, batch.point_offsets_host, rots_dev, px, out),
                   max(a.steps // 4, 2), 1)
        row["torch_scatter_ms"], row["torch_square_px"] = round(ms, 4), 2 * px + 1
        cases.append(row)
        del batch
        torch.cuda.empty_cache()
    mesh = R.MeshBatch([(verts, tris)] * N, dev)
    ms = timed(lambda: r.render(mesh, rotations=rots, out=out), a.steps, a.warmup)
    cases.append({"mesh": "ico20k", "faces": int(len(tris)), "size": S, "N": N, "V": V, "ms": round(ms, 4)})
    if a.table:
        print("%8s %9s %10s %10s %17s" % ("points", "radius px", "depth ms", "normal ms", "torch scatter ms"))
        for c in cases:
            if "points" in c:
                print("%8d %9.2f %10.3f %10.3f %17.3f" % (c["points"], c["radius_px"], c["depth_ms"], c["normal_ms"],
                                                         c["torch_scatter_ms"]))
            else:
                print("mesh %s (%d faces): render %.3f ms" % (c["mesh"], c["faces"], c["ms"]))
    print(json.dumps({"metric": "render_points_ms_per_batch", "unit": "ms", "cases": cases}))


if __name__ == "__main__":
    main()
