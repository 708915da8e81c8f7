"""numpy restatement of the smooth-shading contract (include/gvcnn_hip.h, "meshes in", gv_render_draw_smooth), built on
render_oracle.py and render_ss_oracle.py: coverage, depth, the sample grid and the resolve are theirs; this file adds
the vertex normals (face vectors added per vertex in ascending triangle order) and the colour of a covered sample
(normals interpolated with the integer edge functions at the sample, diffuse + specular).  float32 arrays with one
rounding per operation; a plain loop over corners for the sums, so the order is there to read."""
import numpy as np

import render_oracle as O
import render_ss_oracle as SS

F = np.float32


def face_vectors(w, tris):
    """unnormalised n_t = (w1 - w0) x (w2 - w0), float32 [nt, 3] (the steps of render_oracle.shade_factors)."""
    w0, w1, w2 = w[tris[:, 0]], w[tris[:, 1]], w[tris[:, 2]]
    a, b = w1 - w0, w2 - w0
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(np.float32)


def good_triangles(tris, nv):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    return ((tris >= 0) & (tris < nv)).all(axis=1)


def vertex_normals(w, tris, d, v=None, reverse=False):
    """unit vertex normals float32 [nv, 3]; v: the view whose viewer the face vectors are turned to (two-sided), or
    None.  reverse=True adds the corners of every vertex in DESCENDING triangle order (what the contract does not do:
    for tests that ask whether the order matters)."""
    nv = len(w)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    ok = good_triangles(tris, nv)
    fv = np.zeros((len(tris), 3), np.float32)
    fv[ok] = face_vectors(w, tris[ok])
    if v is not None:
        fwd = O.f32(d["cameras"][v][2])
        turn = O.dot3(fwd, fv[:, 0], fv[:, 1], fv[:, 2]) > 0
        fv = np.where(turn[:, None], -fv, fv)
    g = np.zeros((nv, 3), np.float32)
    seen = np.zeros(nv, bool)
    order = range(len(tris) - 1, -1, -1) if reverse else range(len(tris))
    for t in order:                                                    # ascending triangle id, corner by corner
        if not ok[t]:
            continue
        for i in tris[t]:
            g[i] = g[i] + fv[t] if seen[i] else fv[t]
            seen[i] = True
    nn = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    fine = np.isfinite(nn) & (nn > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = g / np.sqrt(nn)[:, None]
    return np.where(fine[:, None], unit, F(0.0)).astype(np.float32)


def sample_shading(X, Y, tris, normals, flat, face, d, v, S):
    """colours float32 [hits, 3] of the covered samples of one image (face: int32 [S*H, S*W] on the sample grid, in
    np.nonzero order)."""
    ys, xs = np.nonzero(face >= 0)
    t = face[ys, xs].astype(np.int64)
    i0, i1, i2 = tris[t, 0], tris[t, 1], tris[t, 2]
    x0, y0, x1, y1, x2, y2 = X[i0], Y[i0], X[i1], Y[i1], X[i2], Y[i2]
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    flip = area < 0                                                    # the setup swaps vertices 1 and 2: so do we
    x1, x2 = np.where(flip, x2, x1), np.where(flip, x1, x2)
    y1, y2 = np.where(flip, y2, y1), np.where(flip, y1, y2)
    i1, i2 = np.where(flip, i2, i1), np.where(flip, i1, i2)
    area = np.abs(area)
    step = 256 // S
    PX, PY = xs.astype(np.int64) * step + step // 2, ys.astype(np.int64) * step + step // 2

    def edge(ax, ay, bx, by):
        return (bx - ax) * (PY - ay) - (by - ay) * (PX - ax)
    fa = area.astype(np.float32)                                       # int64 -> float32: round to nearest even
    b0 = edge(x1, y1, x2, y2).astype(np.float32) / fa
    b1 = edge(x2, y2, x0, y0).astype(np.float32) / fa
    b2 = edge(x0, y0, x1, y1).astype(np.float32) / fa
    n = (b0[:, None] * normals[i0] + b1[:, None] * normals[i1]) + b2[:, None] * normals[i2]
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    fine = np.isfinite(nn) & (nn > 0)
    two_sided = bool(d["flags"] & 2)
    amb = F(d["ambient"])
    color = O.f32(d["color"])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ln = np.sqrt(nn)
        s = O.dot3(O.f32(d["lights"][v]), n[:, 0], n[:, 1], n[:, 2]) / ln
        h = np.abs(s) if two_sided else np.fmax(s, F(0.0)) if d["diffuse"] == "lambert" else (s + F(1.0)) * F(0.5)
        f = amb + (F(1.0) - amb) * h
        p = O.dot3(O.f32(d["halfs"][v]), n[:, 0], n[:, 1], n[:, 2]) / ln
        p = np.abs(p) if two_sided else np.fmax(p, F(0.0))
        for _ in range(int(d["shininess"]).bit_length() - 1):
            p = p * p
        sp = F(d["specular"]) * p
        smooth = np.fmin(color[None, :] * f[:, None] + sp[:, None], F(1.0))
    return np.where(fine[:, None], smooth, color[None, :] * flat[t][:, None]).astype(np.float32)


def sample_colours(meshes, d, rotations, S):
    """(face_id, depth [N, V, S*H, S*W], colours float32 [N, V, S*H, S*W, 3], status [N]) of a smooth render."""
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
        # a triangle with an index out of range is dropped: it keeps its id and covers nothing
        safe = np.where(good_triangles(tris, len(w))[:, None], tris, 0)
        flat = O.shade_factors(w, safe, d)
        shared = None if d["flags"] & 2 else vertex_normals(w, tris, d)
        for v in range(V):
            X, Y, Z = O.project(w, d["cameras"][v], d)
            fi, dp = SS.raster(X, Y, Z, safe, H, W, S)
            face[m, v], depth[m, v] = fi, dp
            normals = shared if shared is not None else vertex_normals(w, tris, d, v)
            col[m, v][fi >= 0] = sample_shading(X, Y, safe, normals, flat, fi, d, v, S)
    return face, depth, col, status


def render(meshes, d, rotations=None, samples=None):
    """As render_ss_oracle.render for d["shading"] == "smooth": u8, f32q, f32 [N, V, H, W, 3]; face_id, depth
    [N, V, S*H, S*W]; status [N]."""
    assert d["shading"] == "smooth"
    S = int(d.get("samples", 1) if samples is None else samples)
    assert S in (1, 2, 4)
    face, depth, col, status = sample_colours(meshes, d, rotations, S)
    u8 = SS.resolve_u8(SS.split_samples(SS.to_u8(col), S), S)
    return {"face_id": face, "depth": depth, "u8": u8, "f32q": SS.quantised(u8),
            "f32": SS.resolve_f32(SS.split_samples(col, S), S), "status": status}


# ---- the meshes of the smooth tests ---------------------------------------------------------------------------------
def open_patch():
    """a small open mesh: a bent 3 x 3 grid of vertices, 8 triangles, boundary vertices with one to six corners."""
    v = np.array([[x, y, 0.35 * x * x - 0.25 * y] for y in (-1, 0, 1) for x in (-1, 0, 1.2)], np.float32)
    t = [(0, 1, 3), (1, 4, 3), (1, 2, 4), (2, 5, 4), (3, 4, 6), (4, 7, 6), (4, 5, 7), (5, 8, 7)]
    return v, np.array(t, np.int32)


def swap_quad():
    """one quad of two triangles with opposite index order (one of them has negative screen area from either side)."""
    v = np.array([[0, -1, -0.8], [0.3, 1, -1], [-0.2, 1, 0.9], [0.1, -1, 1]], np.float32)
    return v, np.array([(0, 1, 2), (0, 3, 2)], np.int32)


def fan(n=48, seed=3):
    """n thin triangles of very different areas round one apex (vertex 0): the apex normal is a sum of n face vectors
    whose low bits depend on the order of the adds."""
    rng = np.random.RandomState(seed)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, size=n + 1))
    rad = 10.0 ** rng.uniform(-2.0, 0.0, size=n + 1)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.3 * rad * np.sin(3 * ang) - 0.4 * rad], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.2]], rim]).astype(np.float32)
    return v, np.array([(0, i + 1, i + 2) for i in range(n)], np.int32)


def cancelling_sheet():
    """two coincident triangles of opposite winding: every vertex sum is exactly zero (one-sided)."""
    v = np.array([[0, -1, -1], [0, 1, -0.5], [0, 0.2, 1]], np.float32)
    return v, np.array([(0, 1, 2), (0, 2, 1)], np.int32)


def separate_triangles(n=24, seed=5):
    """a triangle soup with no shared vertices: every vertex normal is its own face's."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, size=(n, 1, 3))
    v = (c + rng.uniform(-0.6, 0.6, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)
