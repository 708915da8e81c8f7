"""numpy restatement of the splatting contract (include/gvcnn_hip.h, "points in"): float32 arrays with one rounding per
operation, int64 / uint64 for coverage and keys.  Normalisation, world position and projection are the mesh oracle's
(tests/render_oracle.py), imported, not copied.  Slow and simple: a loop over points, vectorised over the pixels of each
disc's box."""
import numpy as np

from render_oracle import EMPTY, OK, dot3, f32, normalise, project, world

F = np.float32
R_MIN, R_MAX = F(1.0), F(8192.0)                                  # 1/256 pixel; 32 pixels
BG = np.uint64(0xFFFFFFFFFFFFFFFF)


def radii(w, C, d, radius):
    """R (int64, 1/256 pixel) of world points w [n, 3] in camera C: every step rounded, NaN -> R_MIN."""
    r = np.full(len(w), F(radius) * F(d["proj_scale"]), dtype=np.float32)
    if d["flags"] & 1:
        z = dot3(f32(C)[2], w[:, 0], w[:, 1], w[:, 2]) + F(d["persp_dist"])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = r / z
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(np.fmin(np.fmax(f32(r * F(256.0)), R_MIN), R_MAX)).astype(np.int64)


def splat(X, Y, Z, R, ok, H, W):
    """(point_id int32 [H, W], depth uint32 [H, W]) of one image from snapped centres, depths and radii; ok: the points
    that take part."""
    best = np.full((H, W), BG, dtype=np.uint64)
    for i in np.nonzero(ok)[0]:
        x, y, z, r = int(X[i]), int(Y[i]), int(Z[i]), int(R[i])
        px0, px1 = max((x - r + 127) >> 8, 0), min((x + r - 128) >> 8, W - 1)
        py0, py1 = max((y - r + 127) >> 8, 0), min((y + r - 128) >> 8, H - 1)
        if px0 > px1 or py0 > py1:
            continue
        dx = (np.arange(px0, px1 + 1, dtype=np.int64) * 256 + 128 - x)[None, :]
        dy = (np.arange(py0, py1 + 1, dtype=np.int64) * 256 + 128 - y)[:, None]
        cov = dx * dx + dy * dy <= r * r
        key = (np.uint64(z) << np.uint64(32)) | np.uint64(i)
        sub = best[py0:py1 + 1, px0:px1 + 1]
        np.copyto(sub, np.minimum(sub, key), where=cov)
    bg = best == BG
    pid = np.where(bg, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(bg, np.uint64(0xFFFFFFFF), best >> np.uint64(32)).astype(np.uint32)
    return pid, depth


def depth_factor(Z, d):
    """f = ambient + (1 - ambient) * (1 - Z / (2^24 - 1)) per depth (float32)."""
    amb = F(d["ambient"])
    t = f32(Z) / F(16777215.0)
    return amb + (F(1.0) - amb) * (F(1.0) - t)


def normal_colours(n, Z, v, d):
    """colour [k, 3] of splats with world normals n [k, 3] and depths Z [k] in view v: the smooth mode's reflection
    model; a normal without a finite positive length takes the depth factor."""
    color = f32(d["color"])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        good = (nn > 0) & np.isfinite(nn)
        ln = np.sqrt(np.where(good, nn, F(1.0))).astype(np.float32)
        s = dot3(d["lights"][v], n[:, 0], n[:, 1], n[:, 2]) / ln
        two = bool(d["flags"] & 2)
        h = np.abs(s) if two else (np.fmax(s, F(0.0)) if d["diffuse"] == "lambert" else (s + F(1.0)) * F(0.5))
        amb = F(d["ambient"])
        f = amb + (F(1.0) - amb) * h
        sp = np.zeros(len(n), np.float32)
        if d["specular"] > 0:
            t = dot3(d["halfs"][v], n[:, 0], n[:, 1], n[:, 2]) / ln
            p = np.abs(t) if two else np.fmax(t, F(0.0))
            for _ in range(int(np.log2(d["shininess"]))):
                p = p * p
            sp = F(d["specular"]) * p
        lit = np.fmin(color[None, :] * f[:, None] + sp[:, None], F(1.0))
    flat = color[None, :] * depth_factor(Z, d)[:, None]
    return np.where(good[:, None], lit, flat).astype(np.float32)


def render(clouds, d, radius, rotations=None, shading="depth"):
    """clouds: [points [P, 3]] or [(points, normals)]; d: ViewRenderer.descriptor() (point_descriptor() for
    shading="normal"); radius: float32 [N] in normalised units.  Returns dict of numpy arrays [N, V, H, W(, 3)]:
    point_id, depth, u8, f32q, f32, and status [N]."""
    N, V, H, W = len(clouds), d["num_views"], d["height"], d["width"]
    pid = np.full((N, V, H, W), -1, np.int32)
    depth = np.full((N, V, H, W), 0xFFFFFFFF, np.uint32)
    col = np.empty((N, V, H, W, 3), np.float32)
    col[:] = f32(d["background"])
    status = np.zeros(N, np.int32)
    for m, c in enumerate(clouds):
        pts, nrm = c if isinstance(c, tuple) else (c, None)
        pts = f32(pts).reshape(-1, 3)
        if len(pts) == 0:
            status[m] = EMPTY
            continue
        cen, scale, st = normalise(pts, d["fit"])
        status[m] = st
        if st != OK:
            continue
        M = None if rotations is None else rotations[m]
        with np.errstate(over="ignore", invalid="ignore"):
            w = world(pts, cen, scale, M)
        ok = np.isfinite(w).all(axis=1)
        if shading == "normal":
            g = f32(nrm).reshape(-1, 3)
            nw = g if M is None else np.stack([dot3(f32(M)[i], g[:, 0], g[:, 1], g[:, 2]) for i in range(3)], axis=1)
        for v in range(V):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                X, Y, Z = project(np.where(ok[:, None], w, F(0.0)), d["cameras"][v], d)
                R = radii(np.where(ok[:, None], w, F(0.0)), d["cameras"][v], d, radius[m])
            pi, dp = splat(X, Y, Z, R, ok, H, W)
            pid[m, v], depth[m, v] = pi, dp
            hit = pi >= 0
            if shading == "normal":
                col[m, v][hit] = normal_colours(nw[pi[hit]], dp[hit], v, d)
            else:
                col[m, v][hit] = f32(d["color"])[None, :] * depth_factor(dp[hit], d)[:, None]
    u8 = np.clip(np.floor(col * F(255.0) + F(0.5)), 0, 255).astype(np.uint8)
    # one rounding: fma(u8, fp32(1/255), -0.5) (exact in float64: 8 + 24 significant bits)
    f32q = (u8.astype(np.float64) * np.float64(F(1.0 / 255.0)) - 0.5).astype(np.float32)
    return {"point_id": pid, "depth": depth, "u8": u8, "f32q": f32q, "f32": col + F(-0.5), "status": status}
