"""numpy restatement of the supersampled rendering contract (include/gvcnn_hip.h, "meshes in", gv_render_*_ss), built on
render_oracle.py.  The sample-grid buffers of one image are render_oracle.raster(S*X, S*Y, Z, tris, S*H, S*W): scaling
the snapped coordinates by S puts sample (a, b) of pixel (i, j), at 256 i + (256 / S) a + 128 / S, on that function's
pixel centre 256 (S i + a) + 128; edge signs, ties and num div area are unchanged (both scale by S * S) and its bounding
box (S min + 127) >> 8 .. (S max - 128) >> 8 is the contract's sample box.  The resolve is added here: uint64 sums for
the uint8 output, sequential float32 adds for the unquantised one."""
import numpy as np

import render_oracle as O

F = np.float32


def raster(X, Y, Z, tris, H, W, S):
    """(face_id int32, depth uint32) [S*H, S*W] of one image on the sample grid."""
    return O.raster(S * X, S * Y, Z, tris, S * H, S * W)


def to_u8(col):
    return np.clip(np.floor(col * F(255.0) + F(0.5)), 0, 255).astype(np.uint8)


def split_samples(x, S):
    """[..., S*H, S*W, C] -> [..., H, W, S*S, C] with the samples of a pixel in row-major order (b outer, a inner)."""
    lead, (SH, SW, C) = x.shape[:-3], x.shape[-3:]
    x = x.reshape(lead + (SH // S, S, SW // S, S, C))
    n = len(lead)
    x = np.moveaxis(x, n + 1, n + 2)                                   # [..., H, W, b, a, C]
    return x.reshape(lead + (SH // S, SW // S, S * S, C))


def resolve_u8(u8s, S):
    """per-sample uint8 [..., H, W, S*S, C] -> uint8 [..., H, W, C]: (sum + S*S/2) div S*S in exact integers."""
    n = np.uint64(S * S)
    return ((u8s.astype(np.uint64).sum(axis=-2) + n // np.uint64(2)) // n).astype(np.uint8)


def resolve_f32(cols, S):
    """per-sample float32 colours [..., H, W, S*S, C] -> float32 [..., H, W, C]: the samples added in order, one
    rounding per add, times 1 / (S*S) (exact), plus -0.5."""
    cols = cols.astype(np.float32)
    acc = cols[..., 0, :].copy()
    for s in range(1, S * S):
        acc = acc + cols[..., s, :]
    if S > 1:
        acc = acc * F(1.0 / (S * S))
    return acc + F(-0.5)


def quantised(u8):
    """fma(u8, fp32(1/255), -0.5), one rounding (exact in float64: 8 + 24 significant bits)."""
    return (u8.astype(np.float64) * np.float64(F(1.0 / 255.0)) - 0.5).astype(np.float32)


def sample_colours(meshes, d, rotations, S):
    """(face_id, depth [N, V, S*H, S*W], colours float32 [N, V, S*H, S*W, 3], status [N])."""
    N, V, H, W = len(meshes), d["num_views"], d["height"], d["width"]
    face = np.full((N, V, S * H, S * W), -1, np.int32)
    depth = np.full((N, V, S * H, S * W), 0xFFFFFFFF, np.uint32)
    col = np.empty((N, V, S * H, S * W, 3), np.float32)
    col[:] = O.f32(d["background"])
    status = np.zeros(N, np.int32)
    for m, (verts, tris) in enumerate(meshes):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        if len(tris) == 0 or len(verts) == 0:
            status[m] = O.EMPTY
            continue
        c, scale, st = O.normalise(verts, d["fit"])
        status[m] = st
        if st != O.OK:
            continue
        w = O.world(verts, c, scale, None if rotations is None else rotations[m])
        f = O.shade_factors(w, tris, d)
        for v in range(V):
            X, Y, Z = O.project(w, d["cameras"][v], d)
            fi, dp = raster(X, Y, Z, tris, H, W, S)
            face[m, v], depth[m, v] = fi, dp
            hit = fi >= 0
            col[m, v][hit] = O.f32(d["color"])[None, :] * f[fi[hit]][:, None]
    return face, depth, col, status


def render(meshes, d, rotations=None, samples=None):
    """As render_oracle.render with S = samples (default d["samples"]) samples per pixel and axis: u8, f32q, f32
    [N, V, H, W, 3]; face_id, depth [N, V, S*H, S*W]; status [N]."""
    S = int(d.get("samples", 1) if samples is None else samples)
    assert S in (1, 2, 4)
    face, depth, col, status = sample_colours(meshes, d, rotations, S)
    u8 = resolve_u8(split_samples(to_u8(col), S), S)
    return {"face_id": face, "depth": depth, "u8": u8, "f32q": quantised(u8),
            "f32": resolve_f32(split_samples(col, S), S), "status": status}


def tile_counts(meshes, d, rotations=None, samples=None):
    """[N, V, tiles_y, tiles_x] lengths of the 16 x 16-pixel tile lists, binned by the sample box: g0 = max((min + step/2
    - 1) >> log2(step), 0), g1 = min((max - step/2) >> log2(step), S*W - 1), pixels g0 / S .. g1 / S."""
    S = int(d.get("samples", 1) if samples is None else samples)
    N, V, H, W = len(meshes), d["num_views"], d["height"], d["width"]
    step = 256 // S
    sh = step.bit_length() - 1
    out = np.zeros((N, V, (H + 15) // 16, (W + 15) // 16), np.int64)
    for m, (verts, tris) in enumerate(meshes):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        c, scale, st = O.normalise(verts, d["fit"]) if len(tris) and len(verts) else (None, None, O.EMPTY)
        if st != O.OK:
            continue
        w = O.world(verts, c, scale, None if rotations is None else rotations[m])
        for v in range(V):
            X, Y, _ = O.project(w, d["cameras"][v], d)
            x, y = X[tris], Y[tris]
            area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
            gx0 = np.maximum((x.min(1) + step // 2 - 1) >> sh, 0)
            gx1 = np.minimum((x.max(1) - step // 2) >> sh, S * W - 1)
            gy0 = np.maximum((y.min(1) + step // 2 - 1) >> sh, 0)
            gy1 = np.minimum((y.max(1) - step // 2) >> sh, S * H - 1)
            for i in np.nonzero((area != 0) & (gx0 <= gx1) & (gy0 <= gy1))[0]:
                out[m, v, (gy0[i] // S) >> 4:((gy1[i] // S) >> 4) + 1, (gx0[i] // S) >> 4:((gx1[i] // S) >> 4) + 1] += 1
    return out


def thin_strip():
    """a slanted strip about 0.3 pixel wide at 37 x 29 plus a small anchor triangle that fixes the radius."""
    v = np.array([[0, -0.8, -0.9], [0, -0.79, -0.9], [0, 0.5, 0.9], [0, 0.51, 0.9], [0, 1, 0], [0, 0.99, 0.01],
                  [0, 0.99, -0.01]], np.float32)
    return v, np.array([(0, 1, 2), (1, 3, 2), (4, 5, 6)], np.int32)
