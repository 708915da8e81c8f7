"""numpy restatement of the rendering contract (include/gvcnn_hip.h, "meshes in"): float32 arrays with one rounding per
operation (numpy never fuses a multiply and an add), int64 / uint64 for coverage and depth.  Slow and simple: a loop
over triangles, vectorised over the pixels of each triangle's bounding box."""
import numpy as np

F = np.float32
SNAP_LIM = F(262144.0)
OK, EMPTY, ZERO_RADIUS, NONFINITE = 0, 1, 2, 3


def f32(x):
    return np.asarray(x, dtype=np.float32)


def dot3(r, a, b, c):
    return (f32(r[0]) * a + f32(r[1]) * b) + f32(r[2]) * c


def normalise(verts, fit):
    """(c [3], scale, status) of one mesh."""
    v = f32(verts)
    if len(v) == 0:
        return None, None, EMPTY
    c = (v.min(axis=0) + v.max(axis=0)) * F(0.5)
    d = v - c
    r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    r = np.sqrt(F(r2))
    if not np.isfinite(r):
        return c, None, NONFINITE
    if r == 0:
        return c, None, ZERO_RADIUS
    with np.errstate(over="ignore"):
        scale = F(fit) / r
    if not np.isfinite(scale):
        return c, None, NONFINITE
    return c, F(scale), OK


def world(verts, c, scale, M):
    v = f32(verts)
    u = (v - c) * scale
    if M is None:
        return u
    M = f32(M)
    return np.stack([dot3(M[i], u[:, 0], u[:, 1], u[:, 2]) for i in range(3)], axis=1)


def project(w, C, d):
    """snapped X, Y (int64) and Z (int64 < 2^24) of world points w [n, 3] in camera C [3, 3]."""
    C = f32(C)
    q0, q1, q2 = (dot3(C[i], w[:, 0], w[:, 1], w[:, 2]) for i in range(3))
    k, cx, cy = F(d["proj_scale"]), F(d["width"]) * F(0.5), F(d["height"]) * F(0.5)
    if d["flags"] & 1:
        z = q2 + F(d["persp_dist"])
        sx = cx + (q0 * k) / z
        sy = cy - (q1 * k) / z
        t = F(d["depth_a"]) - F(d["depth_b"]) / z
    else:
        sx = cx + q0 * k
        sy = cy - q1 * k
        t = (q2 + F(1.0)) * F(0.5)

    def snap(s):
        return np.rint(np.fmin(np.fmax(s * F(256.0), -SNAP_LIM), SNAP_LIM)).astype(np.int64)
    t = np.fmin(np.fmax(f32(t), F(0.0)), F(1.0))
    return snap(f32(sx)), snap(f32(sy)), np.rint(t * F(16777215.0)).astype(np.int64)


def shade_factors(w, tris, d):
    """flat shading factor f per triangle (float32)."""
    w0, w1, w2 = w[tris[:, 0]], w[tris[:, 1]], w[tris[:, 2]]
    a, b = w1 - w0, w2 - w0
    n0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    n1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    n2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    lt = f32(d["light"])
    nl = (n0 * lt[0] + n1 * lt[1]) + n2 * lt[2]
    nn = (n0 * n0 + n1 * n1) + n2 * n2
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(nn > 0, nl / np.sqrt(nn), F(0.0)).astype(np.float32)
    h = np.abs(s) if d["flags"] & 2 else (s + F(1.0)) * F(0.5)
    amb = F(d["ambient"])
    return amb + (F(1.0) - amb) * h


def owns(ax, ay, bx, by):
    """top-left: positive area in the y-down frame is clockwise on screen; top edges run right, left edges up."""
    dx, dy = bx - ax, by - ay
    return dy < 0 or (dy == 0 and dx > 0)


def raster(X, Y, Z, tris, H, W):
    """(face_id int32 [H, W], depth uint32 [H, W]) of one image from snapped vertices."""
    best = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    for tid, (i0, i1, i2) in enumerate(tris):
        x0, y0, z0 = int(X[i0]), int(Y[i0]), int(Z[i0])
        x1, y1, z1 = int(X[i1]), int(Y[i1]), int(Z[i1])
        x2, y2, z2 = int(X[i2]), int(Y[i2]), int(Z[i2])
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        if area < 0:
            x1, y1, z1, x2, y2, z2 = x2, y2, z2, x1, y1, z1
            area = -area
        px0 = max((min(x0, x1, x2) + 127) >> 8, 0)
        px1 = min((max(x0, x1, x2) - 128) >> 8, W - 1)
        py0 = max((min(y0, y1, y2) + 127) >> 8, 0)
        py1 = min((max(y0, y1, y2) - 128) >> 8, H - 1)
        if px0 > px1 or py0 > py1:
            continue
        PX = (np.arange(px0, px1 + 1, dtype=np.int64) * 256 + 128)[None, :]
        PY = (np.arange(py0, py1 + 1, dtype=np.int64) * 256 + 128)[:, None]

        def edge(ax, ay, bx, by):
            return (bx - ax) * (PY - ay) - (by - ay) * (PX - ax)
        e0, e1, e2 = edge(x1, y1, x2, y2), edge(x2, y2, x0, y0), edge(x0, y0, x1, y1)
        cov = (((e0 > 0) | ((e0 == 0) & owns(x1, y1, x2, y2))) & ((e1 > 0) | ((e1 == 0) & owns(x2, y2, x0, y0))) &
               ((e2 > 0) | ((e2 == 0) & owns(x0, y0, x1, y1))))
        if not cov.any():
            continue
        num = (e0.astype(np.uint64) * np.uint64(z0) + e1.astype(np.uint64) * np.uint64(z1) +
               e2.astype(np.uint64) * np.uint64(z2))
        Zp = num // np.uint64(area)
        key = (Zp << np.uint64(32)) | np.uint64(tid)
        sub = best[py0:py1 + 1, px0:px1 + 1]
        np.copyto(sub, np.minimum(sub, key), where=cov)
    bg = best == np.uint64(0xFFFFFFFFFFFFFFFF)
    face = np.where(bg, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(bg, np.uint64(0xFFFFFFFF), best >> np.uint64(32)).astype(np.uint32)
    return face, depth


def tile_counts(meshes, d, rotations=None):
    """[N, V, tiles_y, tiles_x] triangle counts of the 16 x 16 tile lists, binned as the kernels bin (pixel-centre bbox
    of every triangle that covers one): how far a case drives the multi-pass tile loop."""
    N, V, H, W = len(meshes), d["num_views"], d["height"], d["width"]
    out = np.zeros((N, V, (H + 15) // 16, (W + 15) // 16), np.int64)
    for m, (verts, tris) in enumerate(meshes):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        c, scale, st = normalise(verts, d["fit"]) if len(tris) and len(verts) else (None, None, EMPTY)
        if st != OK:
            continue
        w = world(verts, c, scale, None if rotations is None else rotations[m])
        for v in range(V):
            X, Y, _ = project(w, d["cameras"][v], d)
            x, y = X[tris], Y[tris]
            area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
            px0 = np.maximum((x.min(1) + 127) >> 8, 0)
            px1 = np.minimum((x.max(1) - 128) >> 8, W - 1)
            py0 = np.maximum((y.min(1) + 127) >> 8, 0)
            py1 = np.minimum((y.max(1) - 128) >> 8, H - 1)
            for i in np.nonzero((area != 0) & (px0 <= px1) & (py0 <= py1))[0]:
                out[m, v, py0[i] >> 4:(py1[i] >> 4) + 1, px0[i] >> 4:(px1[i] >> 4) + 1] += 1
    return out


def render(meshes, d, rotations=None):
    """meshes [(verts, tris)], d: ViewRenderer.descriptor().  Returns dict of numpy arrays [N, V, H, W(, 3)]:
    face_id, depth, u8, f32q (quantised fp32), f32 (exact), and status [N]."""
    N, V, H, W = len(meshes), d["num_views"], d["height"], d["width"]
    face = np.full((N, V, H, W), -1, np.int32)
    depth = np.full((N, V, H, W), 0xFFFFFFFF, np.uint32)
    col = np.empty((N, V, H, W, 3), np.float32)
    col[:] = f32(d["background"])
    status = np.zeros(N, np.int32)
    for m, (verts, tris) in enumerate(meshes):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        if len(tris) == 0 or len(verts) == 0:
            status[m] = EMPTY
            continue
        c, scale, st = normalise(verts, d["fit"])
        status[m] = st
        if st != OK:
            continue
        w = world(verts, c, scale, None if rotations is None else rotations[m])
        f = shade_factors(w, tris, d)
        for v in range(V):
            X, Y, Z = project(w, d["cameras"][v], d)
            fi, dp = raster(X, Y, Z, tris, H, W)
            face[m, v], depth[m, v] = fi, dp
            hit = fi >= 0
            col[m, v][hit] = f32(d["color"])[None, :] * f[fi[hit]][:, None]
    u8 = np.clip(np.floor(col * F(255.0) + F(0.5)), 0, 255).astype(np.uint8)
    # one rounding: fma(u8, fp32(1/255), -0.5) (exact in float64: 8 + 24 significant bits)
    f32q = (u8.astype(np.float64) * np.float64(F(1.0 / 255.0)) - 0.5).astype(np.float32)
    return {"face_id": face, "depth": depth, "u8": u8, "f32q": f32q, "f32": col + F(-0.5),
            "status": status}
