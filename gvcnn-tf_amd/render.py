"""Meshes in: render a batch of triangle meshes into the backbone's input views on the device.

    verts, tris = load_off("chair_0001.off")
    batch = MeshBatch([(verts, tris), ...], device)              # uploaded once
    r = ViewRenderer(12, 224, 224)                               # obj2png.py's cameras: azimuth 30*(i+1), elevation 30
    views = r.render(batch)                                      # [N, 12, 224, 224, 3] fp32 in [-0.5, 0.5]
    views = r.render(batch, rotations=random_rotations(len(batch), "z", seed))   # augmentation

The rasteriser is csrc/render.hip; its contract (written out in include/gvcnn_hip.h, "meshes in") makes every pixel
reproducible bit for bit:
  - per mesh, fp32 with every step rounded: c = bbox midpoint, r = max |v - c| (correctly rounded sqrt),
    u = (v - c) * (fit / r); optional rotation w = M u ([N, 3, 3] fp32 rotation matrices, checked on the host);
  - cameras as matplotlib's view_init(elev, azim) with +z up, looking at the origin; C_v [3, 3] (rows right, up,
    forward) built in float64 on the host and rounded to fp32.  fov = 0: orthographic, the unit sphere on the shorter
    image side; fov > 0: perspective with the eye at 1/sin(fov/2), the unit sphere tangent to the frustum;
  - screen coordinates snapped to 1/256 pixel (round to nearest even), pixel centres at (i + 0.5, j + 0.5), row 0 on
    top; integer edge functions with the top-left rule (top and left edges own the pixel centres on them); 24-bit
    depth affine in screen space; the pixel keeps the smallest (depth << 32 | triangle id), so equal depths go to the
    lower id and scheduling never matters;
  - flat shading by the world-space face normal n = (w1-w0) x (w2-w0) and the light l: s = n.l / |n|,
    f = ambient + (1 - ambient) * (s + 1) / 2 (matplotlib's _shade_colors with ambient 0.3; two_sided: |s|),
    colour = color * f on a background colour;
  - uint8 = floor(c * 255 + 0.5); quantize=True gives fma(uint8, 1/255, -0.5), rounded once (what the record pipeline's
    gv_preprocess_views computes from a PNG, so a render equals its own PNG round trip); quantize=False gives c - 0.5;
  - samples=S (1, 2 or 4): S x S coverage and depth samples per pixel on a regular grid ((256 / S) * a + 128 / S in
    1/256 pixel), each treated as a pixel centre above and resolved in the same launch: the uint8 pixel is the rounded
    mean of the samples' uint8 values, the unquantised one the mean of their colours added in row-major order, - 0.5.
  - shading="smooth" (Phong reflection on interpolated normals; every step fp32, rounded on its own, still bit-exact
    against tests/render_smooth_oracle.py): the face vectors n_t = (w1-w0) x (w2-w0), unnormalised (area weights), are
    added per vertex over its corners in ascending triangle order, starting from the first (MeshBatch.adjacency: a CSR
    built on the host with a stable sort, uploaded once; one thread per vertex gathers, no atomics) and normalised,
    (0, 0, 0) when the sum has no finite positive length.  two_sided=True first turns every face vector towards the
    viewer (negated when forward_v . n_t > 0), so there is one normal table per view.  Per covered sample the resolve
    recomputes the winning triangle's setup and its three integer edge functions e_k at the sample; b_k = float(e_k) /
    float(area), n = (b0*ga + b1*gb) + b2*gc with the normals following the setup's swap of vertices 1 and 2: affine in
    screen space like the depth, NOT perspective-correct.  s = (n.l_v) / |n|; h = (s+1)/2 (diffuse="wrap"), max(s, 0)
    ("lambert") or |s| (two_sided); f = ambient + (1-ambient) * h; t = max((n.m_v) / |n|, 0) (|.| when two_sided),
    p = t squared log2(shininess) times; channel = min(color * f + specular * p, 1).  l_v is the world light or, with
    light="camera", the unit vector from the origin to view v's eye; m_v = normalize(l_v + eye_v), float64 on the host,
    rounded to fp32.  A sample whose interpolated normal has no finite positive length takes its triangle's flat
    factor (the table of the flat mode: wrap or |s|, the world light; DEFAULT_LIGHT with light="camera").  With
    samples > 1 every sample is shaded at its own position.
Points in (csrc/render_points.hip; contract: include/gvcnn_hip.h, "points in"; restated in tests/render_points_oracle.py):

    pts = load_points("scan.xyz")                                # [P, 3], or (points, normals) from six columns
    pts, normals = sample_surface(verts, tris, 20000, seed=0)    # ... or a cloud from a mesh
    batch = PointBatch([pts, ...], device)
    views = r.render_points(batch)                               # the same [N, 12, 224, 224, 3]

  - the cloud is normalised, rotated, projected and snapped exactly as a mesh's vertices are; point i becomes a disc
    around its snapped centre, parallel to the screen, at the point's 24-bit depth: R = rint(min(max((radius * k) * 256,
    1), 8192)) in 1/256 pixel (perspective: (radius * k) / z), radius per cloud in normalised units ("auto":
    auto_point_radius); pixel centre P is covered when |P - centre|^2 <= R^2 in int64 (the boundary belongs to the
    disc); the pixel keeps the smallest (depth << 32 | point id).  A disc under about 0.71 pixel can miss every centre.
  - shading="depth": f = ambient + (1 - ambient) * (1 - Z / (2^24 - 1)), colour = color * f, nearer is brighter;
    shading="normal": the reflection model above on the point's own (rotated) normal, with l_v and m_v as above; a
    normal without a finite positive length takes the depth factor.  One sample per pixel only.
  - a cloud without normals (a raw scan) gets them on the device: batch.estimate_normals(k=16, orient="outward") or
    PointBatch(clouds, device, estimate_normals=16) (csrc/point_normals.hip; contract: include/gvcnn_hip.h, "points in",
    normal estimation; restated in tests/point_normals_oracle.py): per point the exact k nearest neighbours within its
    cloud (fp32 squared distances, ties to the lower id), their fp64 covariance, its smallest eigenvector by cyclic
    Jacobi, turned away from the bounding box's centre ("outward"), towards a sensor position ("viewpoint") or so that
    its largest component is positive ("none").  Bit for bit the same whatever the batch, the grid or the schedule.
  - a raw scan is cleaned on the device first: batch.voxel_downsample(voxel) keeps the centroid of every occupied voxel,
    batch.remove_outliers(k=16, std_ratio=2.0) drops the points whose mean distance to their k nearest neighbours lies
    more than std_ratio standard deviations above the cloud's mean (csrc/point_clean.hip; contract: include/gvcnn_hip.h,
    "points in", cleaning; restated in tests/points_clean_oracle.py).  Each returns a new PointBatch that every call
    above takes; PointBatch.from_device wraps tensors that are on the device already.
  - a scan that comes as several partial clouds is put together on the device first: moved = piece.register(first) aligns
    cloud m of one batch to cloud m of another by point-to-point ICP (csrc/point_register.hip; contract: include/gvcnn_hip.h,
    "points in", registration; restated in tests/points_register_oracle.py): the exact nearest target point of every moved
    source point, fp64 tree sums, Horn's quaternion by cyclic Jacobi, no read-back between rounds;
    PointBatch.merged(first, moved) concatenates pair by pair, and voxel_downsample removes the doubled points.
The defaults are the reference's renders (data_utils/obj2png.py): 8 views at azimuth 45 * (i + 1) there, C0 blue
(31, 119, 180) / 255 on white, the light of LightSource(azdeg=225, altdeg=19.4712).
"""
import math
import numbers

import numpy as np
import torch

from . import _lib
from . import model as _model

MAX_SIDE = 512
MAX_VIEWS = 64
MAX_TRIS = 1 << 24
MAX_POINTS = 1 << 24
DEFAULT_COLOR = (31 / 255.0, 119 / 255.0, 180 / 255.0)         # matplotlib C0
DEFAULT_BACKGROUND = (1.0, 1.0, 1.0)
DEFAULT_MAX_WORKSPACE = 2 << 30
ROTATION_TOL = 1e-4                                           # |M M^T - I| bound of a rotation matrix
STATUS = {_lib.GV_RENDER_OK: "ok", _lib.GV_RENDER_EMPTY: "empty", _lib.GV_RENDER_ZERO_RADIUS: "zero radius",
          _lib.GV_RENDER_NONFINITE: "non-finite radius", _lib.GV_RENDER_TOO_LARGE: "more than 2^24 triangles",
          _lib.GV_RENDER_BAD_OFFSETS: "bad offsets"}


def light_direction(azdeg=225.0, altdeg=19.4712):
    """matplotlib.colors.LightSource(azdeg, altdeg).direction, float64."""
    az, alt = math.radians(90.0 - azdeg), math.radians(altdeg)
    return (math.cos(az) * math.cos(alt), math.sin(az) * math.cos(alt), math.sin(alt))


DEFAULT_LIGHT = light_direction()


def _device(device=None):
    """The device with its index resolved ('cuda' -> 'cuda:<current>'), so two spellings of one device compare equal."""
    d = _model._dev(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def check_rotations(rotations, n=None):
    """rotations [n, 3, 3] -> float32 numpy, checked on the host: finite, orthonormal (max |M M^T - I| <= 1e-4) and
    det > 0.  The contract's bounds (every vertex inside the unit sphere, in front of a perspective eye) hold only for
    rotations; ValueError otherwise.  A device tensor is copied to the host for the check (one read)."""
    r = rotations.detach().cpu().numpy() if torch.is_tensor(rotations) else np.asarray(rotations)
    if r.ndim != 3 or r.shape[1:] != (3, 3) or (n is not None and r.shape[0] != n):
        raise ValueError("rotations must be [%s, 3, 3], got %s" % ("n" if n is None else n, r.shape))
    r = r.astype(np.float32)
    m = r.astype(np.float64)
    if not np.isfinite(m).all():
        raise ValueError("rotations must be finite")
    err = np.abs(m @ m.transpose(0, 2, 1) - np.eye(3)).max() if len(m) else 0.0
    if err > ROTATION_TOL or (len(m) and np.linalg.det(m).min() <= 0):
        raise ValueError("rotations must be rotation matrices (orthonormal, det +1): max |M M^T - I| = %.3g" % err)
    return r


# ---- mesh files ------------------------------------------------------------------------------------------------------
def _fan(poly):
    return [(poly[0], poly[i], poly[i + 1]) for i in range(1, len(poly) - 1)]


def _finish(verts, tris, what):
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("%s: a face index is outside [0, %d)" % (what, len(v)))
    return v, t.astype(np.int32)


def _lines(text):
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if line:
            yield line


def parse_off(text, what="OFF"):
    """OFF text -> (verts float32 [nv, 3], tris int32 [nt, 3]).  ModelNet quirks: 'OFF' glued to the counts
    ('OFF1234 5678 0'), comments, blank lines, polygons (fan-triangulated), colour tokens after a face."""
    toks = _lines(text)
    try:
        head = next(toks)
    except StopIteration:
        raise ValueError("%s: empty file" % what)
    if not head.startswith("OFF"):
        raise ValueError("%s: no OFF header" % what)
    rest = head[3:].split()
    if not rest:
        try:
            rest = next(toks).split()
        except StopIteration:
            raise ValueError("%s: truncated (no counts)" % what)
    try:
        nv, nf = int(rest[0]), int(rest[1])
    except (IndexError, ValueError):
        raise ValueError("%s: bad counts line" % what)
    if nv < 0 or nf < 0:
        raise ValueError("%s: negative counts" % what)
    verts, tris = [], []
    try:
        for _ in range(nv):
            p = next(toks).split()
            if len(p) < 3:
                raise ValueError("%s: a vertex line has fewer than 3 values" % what)
            verts.append([float(p[0]), float(p[1]), float(p[2])])
        for _ in range(nf):
            p = next(toks).split()
            k = int(p[0])
            if k < 3 or len(p) < 1 + k:
                raise ValueError("%s: a face line is short" % what)
            poly = [int(x) for x in p[1:1 + k]]              # anything after: colour tokens
            if min(poly) < 0 or max(poly) >= nv:
                raise ValueError("%s: a face index is outside [0, %d)" % (what, nv))
            tris.extend(_fan(poly))
    except StopIteration:
        raise ValueError("%s: truncated (expected %d vertices and %d faces)" % (what, nv, nf))
    return _finish(verts, tris, what)


def parse_obj(text, what="OBJ"):
    """OBJ text -> (verts, tris): 'v x y z', 'f a b c ...' with a, a/b, a/b/c or a//c, 1-based or negative (relative)
    indices; polygons are fan-triangulated (ObjFile.QuadToTria does the same for quads)."""
    verts, tris = [], []
    for line in _lines(text):
        p = line.split()
        if p[0] == "v":
            if len(p) < 4:
                raise ValueError("%s: a vertex line has fewer than 3 values" % what)
            verts.append([float(p[1]), float(p[2]), float(p[3])])
        elif p[0] == "f":
            if len(p) < 4:
                raise ValueError("%s: a face has fewer than 3 vertices" % what)
            poly = []
            for tok in p[1:]:
                i = int(tok.split("/")[0])
                j = i - 1 if i > 0 else len(verts) + i
                if i == 0 or not 0 <= j < len(verts):
                    raise ValueError("%s: face index %d is outside the %d vertices read so far" % (what, i, len(verts)))
                poly.append(j)
            tris.extend(_fan(poly))
    return _finish(verts, tris, what)


def load_off(path):
    with open(path) as f:
        return parse_off(f.read(), str(path))


def load_obj(path):
    with open(path) as f:
        return parse_obj(f.read(), str(path))


def load_mesh(path):
    p = str(path).lower()
    if p.endswith(".off"):
        return load_off(path)
    if p.endswith(".obj"):
        return load_obj(path)
    raise ValueError("unknown mesh format: %s" % path)


# ---- packing -------------------------------------------------------------------------------------------------------
def pack_meshes(meshes):
    """[(verts [nv, 3], tris [nt, 3]), ...] -> dict of host arrays: verts float32 [sum nv, 3], tris int32 [sum nt, 3]
    (local indices), vert_offsets / tri_offsets int64 [N + 1].  Every mesh is checked here, before any upload:
    finite vertices, integer indices in [0, nv), at most 2^24 triangles."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("no meshes")
    vs, ts = [], []
    for i, m in enumerate(meshes):
        try:
            v, t = m
        except (TypeError, ValueError):
            raise ValueError("mesh %d is not a (verts, tris) pair" % i)
        v = np.asarray(v)
        t = np.asarray(t)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError("mesh %d: verts must be [nv, 3], got %s" % (i, v.shape))
        if t.size == 0:
            t = t.reshape(0, 3)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("mesh %d: tris must be [nt, 3], got %s" % (i, t.shape))
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError("mesh %d: tris must be integers" % i)
        with np.errstate(over="ignore"):
            v = v.astype(np.float32)
        if not np.isfinite(v).all():
            raise ValueError("mesh %d: non-finite vertex" % i)
        if t.size and (t.min() < 0 or t.max() >= len(v)):
            raise ValueError("mesh %d: a triangle index is outside [0, %d)" % (i, len(v)))
        if len(t) > MAX_TRIS:
            raise ValueError("mesh %d: %d triangles (at most 2^24)" % (i, len(t)))
        vs.append(v)
        ts.append(t.astype(np.int32))
    vo = np.zeros(len(meshes) + 1, np.int64)
    to = np.zeros(len(meshes) + 1, np.int64)
    vo[1:] = np.cumsum([len(v) for v in vs])
    to[1:] = np.cumsum([len(t) for t in ts])
    return {"verts": np.concatenate(vs).reshape(-1, 3), "tris": np.concatenate(ts).reshape(-1, 3),
            "vert_offsets": vo, "tri_offsets": to}


def vertex_adjacency(tris, nv):
    """Vertex-to-corner adjacency of one mesh as a CSR: (offsets int64 [nv + 1], triangle ids int32 [corners]); vertex
    i is named by the corners of triangles ids[offsets[i]:offsets[i + 1]], ascending (a triangle that names it twice
    appears twice).  A stable sort of the flattened index array; corners of a triangle with any index outside [0, nv)
    are left out (the rasteriser drops those triangles)."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < nv)).all(axis=1)
    tid = np.repeat(np.arange(len(t), dtype=np.int64)[ok], 3)
    key = t[ok].reshape(-1)
    order = np.argsort(key, kind="stable")
    off = np.zeros(nv + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(key, minlength=nv)[:nv]) if nv else 0
    return off, tid[order].astype(np.int32)


class MeshBatch:
    """Meshes packed and uploaded once (a dataset held on the device can be re-rendered every epoch)."""

    def __init__(self, meshes, device=None):
        p = pack_meshes(meshes)
        self.device = _device(device)
        self.n = len(p["vert_offsets"]) - 1
        self.vert_offsets_host, self.tri_offsets_host = p["vert_offsets"], p["tri_offsets"]
        self.num_tris = np.diff(p["tri_offsets"])
        # one element at least: an empty tensor has no address to hand to the library
        v = p["verts"] if len(p["verts"]) else np.zeros((1, 3), np.float32)
        t = p["tris"] if len(p["tris"]) else np.zeros((1, 3), np.int32)
        self.verts = torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        self.tris = torch.from_numpy(np.ascontiguousarray(t)).to(self.device)
        self.vert_offsets = torch.from_numpy(p["vert_offsets"]).to(self.device)
        self.tri_offsets = torch.from_numpy(p["tri_offsets"]).to(self.device)
        self._adjacency_host = self._adjacency = None

    def adjacency_host(self):
        """(corner_offsets int64 [sum nv + 1], corner_tris int32 [corners]): vertex_adjacency of every mesh, the offsets
        running on through the packed vertices.  Built once, on first use, from the triangles the device holds."""
        if self._adjacency_host is None:
            vo, to = self.vert_offsets_host, self.tri_offsets_host
            tris = self.tris.cpu().numpy()
            offs, ids, base = [np.zeros(1, np.int64)], [], 0
            for m in range(self.n):
                off, tid = vertex_adjacency(tris[to[m]:to[m + 1]], int(vo[m + 1] - vo[m]))
                offs.append(off[1:] + base)
                ids.append(tid)
                base += len(tid)
            self._adjacency_host = (np.concatenate(offs), np.concatenate(ids) if ids else np.zeros(0, np.int32))
        return self._adjacency_host

    def adjacency(self):
        """The adjacency on the device (uploaded once, on the first smooth render)."""
        if self._adjacency is None:
            off, tid = self.adjacency_host()
            tid = tid if len(tid) else np.zeros(1, np.int32)             # an address to hand over
            self._adjacency = (torch.from_numpy(off).to(self.device), torch.from_numpy(tid).to(self.device))
        return self._adjacency

    def __len__(self):
        return self.n

    def group(self, a, b):
        """The C-ABI arguments of meshes [a, b): pointers into the packed arrays (no copy)."""
        vo, to = self.vert_offsets_host, self.tri_offsets_host
        return (self.verts.data_ptr() + int(vo[a]) * 12, self.vert_offsets.data_ptr() + a * 8,
                self.tris.data_ptr() + int(to[a]) * 12, self.tri_offsets.data_ptr() + a * 8, b - a,
                int(vo[b] - vo[a]), int(to[b] - to[a]), int(self.num_tris[a:b].max()))

    def group_adjacency(self, a, b):
        """The adjacency arguments of meshes [a, b): (corner_offsets pointer, corner_tris pointer, corners).  The
        library re-bases the offsets by their first entry, as it does the mesh offsets."""
        off, tid = self.adjacency()
        vo, co = self.vert_offsets_host, self.adjacency_host()[0]
        c0, c1 = int(co[vo[a]]), int(co[vo[b]])
        return off.data_ptr() + int(vo[a]) * 8, tid.data_ptr() + c0 * 4, c1 - c0


# ---- point clouds ----------------------------------------------------------------------------------------------------
def load_points(path):
    """A point cloud file -> points float32 [P, 3], or (points, normals) when the file has six columns (x y z nx ny nz,
    the resampled ModelNet40 layout).  .xyz / .pts / .txt: one point per line, values separated by whitespace or commas,
    '#' starts a comment; .npy: an array [P, 3] or [P, 6].  ValueError for anything else: an unknown extension, no
    points, a line with another number of columns, a token that is no number, a non-finite value."""
    p = str(path).lower()
    if p.endswith(".npy"):
        try:
            a = np.load(path, allow_pickle=False)
        except Exception as e:
            raise ValueError("%s: not a readable .npy array (%s)" % (path, e))
        if a.ndim != 2 or a.shape[1] not in (3, 6) or not (np.issubdtype(a.dtype, np.floating)
                                                            or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s: expected a numeric array [P, 3] or [P, 6], got %s %s" % (path, a.dtype, a.shape))
    elif p.endswith((".xyz", ".pts", ".txt")):
        with open(path) as f:
            rows = [line.replace(",", " ").split() for line in _lines(f.read())]
        if not rows:
            raise ValueError("%s: no points" % path)
        cols = len(rows[0])
        if cols not in (3, 6):
            raise ValueError("%s: %d columns (expected 3 or 6)" % (path, cols))
        for i, r in enumerate(rows):
            if len(r) != cols:
                raise ValueError("%s: point %d has %d columns, the first has %d" % (path, i, len(r), cols))
        try:
            a = np.array(rows, dtype=np.float64)
        except ValueError:
            raise ValueError("%s: a value is not a number" % path)
    else:
        raise ValueError("unknown point cloud format: %s" % path)
    if len(a) == 0:
        raise ValueError("%s: no points" % path)
    with np.errstate(over="ignore"):
        a = a.astype(np.float32)
    if not np.isfinite(a).all():
        raise ValueError("%s: non-finite value" % path)
    if a.shape[1] == 3:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:])


def sample_surface(verts, tris, n, seed=0, return_faces=False):
    """n points on the surface of a mesh, uniform by area, and the unit normal of the face each one lies on (winding
    defined): (points float32 [n, 3], normals float32 [n, 3]), with return_faces also the face ids int64 [n].  Host
    numpy in float64, np.random.RandomState(seed): the same arguments give the same cloud.  How a mesh becomes a cloud."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    n = int(n)
    if v.ndim != 2 or v.shape[1] != 3 or not np.isfinite(v).all():
        raise ValueError("verts must be finite [nv, 3]")
    if n < 0 or len(t) == 0 or t.min() < 0 or t.max() >= len(v):
        raise ValueError("sample_surface needs n >= 0 and triangles with indices in [0, %d)" % len(v))
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cr = np.cross(b - a, c - a)
    area2 = np.linalg.norm(cr, axis=1)
    if not area2.sum() > 0:
        raise ValueError("the mesh has no area")
    rng = np.random.RandomState(seed)
    cdf = np.cumsum(area2) / area2.sum()
    f = np.minimum(np.searchsorted(cdf, rng.uniform(size=n), side="right"), len(t) - 1)
    f = np.where(area2[f] > 0, f, int(np.argmax(area2)))             # (a rounding step onto a zero-area face)
    s, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    w0, w1, w2 = 1.0 - s, s * (1.0 - r2), s * r2
    p = w0[:, None] * a[f] + w1[:, None] * b[f] + w2[:, None] * c[f]
    out = (p.astype(np.float32), (cr[f] / area2[f][:, None]).astype(np.float32))
    return out + (f,) if return_faces else out


def auto_point_radius(P, fit, k):
    """The radius="auto" of render_points for a cloud of P points, in normalised units: min(max(2 * fit / sqrt(P), 1 / k),
    32 / k), float64 rounded to fp32.  2 * fit / sqrt(P) is about the spacing of P points spread over a disc of radius
    fit (twice it closes the gaps of an uneven sampling); the clamps keep the disc between 1 and 32 pixels.  fit, k: the
    renderer's descriptor()['fit'] and ['proj_scale']."""
    return np.float32(min(max(2.0 * float(fit) / math.sqrt(max(int(P), 1)), 1.0 / float(k)), 32.0 / float(k)))


def pack_points(clouds):
    """[points [P, 3] or (points, normals [P, 3]), ...] -> dict of host arrays: points float32 [sum P, 3], normals float32
    [sum P, 3] or None, point_offsets int64 [N + 1].  A cloud with normals is a tuple; normals are all or none across
    the list.  Every cloud is checked here, before any upload: shapes, finite values, at most 2^24 points."""
    clouds = list(clouds)
    if not clouds:
        raise ValueError("no point clouds")
    ps, ns = [], []
    for i, c in enumerate(clouds):
        g = None
        if isinstance(c, tuple):
            if len(c) != 2:
                raise ValueError("cloud %d is not points or a (points, normals) pair" % i)
            c, g = c
        p = np.asarray(c)
        if p.size == 0:
            p = p.reshape(0, 3)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("cloud %d: points must be [P, 3], got %s" % (i, p.shape))
        with np.errstate(over="ignore"):
            p = p.astype(np.float32)
        if not np.isfinite(p).all():
            raise ValueError("cloud %d: non-finite point" % i)
        if len(p) > MAX_POINTS:
            raise ValueError("cloud %d: %d points (at most 2^24)" % (i, len(p)))
        if g is not None:
            g = np.asarray(g)
            if g.size == 0:
                g = g.reshape(0, 3)
            if g.shape != p.shape:
                raise ValueError("cloud %d: normals must be %s like the points, got %s" % (i, p.shape, g.shape))
            with np.errstate(over="ignore"):
                g = g.astype(np.float32)
            if not np.isfinite(g).all():
                raise ValueError("cloud %d: non-finite normal" % i)
        if ns and (g is None) != (ns[0] is None):
            raise ValueError("cloud %d: normals are all or none across a batch" % i)
        ps.append(p)
        ns.append(g)
    po = np.zeros(len(clouds) + 1, np.int64)
    po[1:] = np.cumsum([len(p) for p in ps])
    return {"points": np.concatenate(ps).reshape(-1, 3),
            "normals": None if ns[0] is None else np.concatenate(ns).reshape(-1, 3), "point_offsets": po}


NORMALS_MIN_K, NORMALS_MAX_K, NORMALS_MAX_GRID = 3, 32, 128
NORMALS_ORIENT = {"none": _lib.GV_NORMALS_ORIENT_NONE, "outward": _lib.GV_NORMALS_ORIENT_OUTWARD,
                  "viewpoint": _lib.GV_NORMALS_ORIENT_VIEWPOINT}


def _check_k(k, lo, hi, what):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not lo <= k <= hi:
        raise ValueError("%s: k must be an integer in [%d, %d]" % (what, lo, hi))
    return int(k)


def _check_normals_k(k):
    return _check_k(k, NORMALS_MIN_K, NORMALS_MAX_K, "estimate_normals")


def _check_grid(grid, what):
    if grid is None:
        return 0
    if isinstance(grid, bool) or not isinstance(grid, numbers.Integral) or not 1 <= grid <= NORMALS_MAX_GRID:
        raise ValueError("%s: grid must be None (auto) or an integer in [1, %d]" % (what, NORMALS_MAX_GRID))
    return int(grid)


def _check_normals_args(k, orient, viewpoint, grid):
    """(k, GV_NORMALS_ORIENT_* code, viewpoint float32 [3] or None, grid_cells) of estimate_normals, or ValueError."""
    k = _check_normals_k(k)
    if not isinstance(orient, str) or orient not in NORMALS_ORIENT:
        raise ValueError("estimate_normals: orient must be one of %s" % sorted(NORMALS_ORIENT))
    if (viewpoint is not None) != (orient == "viewpoint"):
        raise ValueError("estimate_normals: a viewpoint goes with orient='viewpoint', and only with it")
    if viewpoint is not None:
        try:
            with np.errstate(over="ignore"):
                viewpoint = np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).astype(np.float32))
        except (TypeError, ValueError):
            raise ValueError("estimate_normals: viewpoint must be three finite numbers")
        if viewpoint.shape != (3,) or not np.isfinite(viewpoint).all():
            raise ValueError("estimate_normals: viewpoint must be three finite numbers")
    return k, NORMALS_ORIENT[orient], viewpoint, _check_grid(grid, "estimate_normals")


CLEAN_MIN_K, CLEAN_MAX_K = 1, 32


def _check_outlier_args(k, std_ratio, grid):
    """(k, std_ratio as float32, grid_cells) of remove_outliers, or ValueError."""
    k = _check_k(k, CLEAN_MIN_K, CLEAN_MAX_K, "remove_outliers")
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, numbers.Real):
        raise ValueError("remove_outliers: std_ratio must be a finite number >= 0")
    with np.errstate(over="ignore"):
        ratio = np.float32(std_ratio)
    if not (np.isfinite(ratio) and ratio >= 0):
        raise ValueError("remove_outliers: std_ratio must be a finite number >= 0")
    return int(k), ratio, _check_grid(grid, "remove_outliers")


def _check_voxel_args(voxel, relative, n):
    """(voxel float32 [n], relative 0 / 1) of voxel_downsample, or ValueError.  A size is a finite number > 0: the
    passthrough clauses of the contract are for sizes that turn bad on the device (relative to a cloud without extent)."""
    if not isinstance(relative, (bool, np.bool_)):
        raise ValueError("voxel_downsample: relative must be True or False")
    try:
        with np.errstate(over="ignore"):
            v = np.asarray(voxel, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError("voxel_downsample: voxel must be a number or one number per cloud")
    if isinstance(voxel, (bool, np.bool_)) or v.ndim > 1 or (v.ndim == 1 and len(v) != n):
        raise ValueError("voxel_downsample: voxel must be a number or one number per cloud (%d)" % n)
    v = np.ascontiguousarray(np.broadcast_to(v, (n,)))
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError("voxel_downsample: a voxel size must be finite and > 0")
    return v, int(bool(relative))


def _check_register_args(n, iterations, max_distance, tolerance, init, grid):
    """(iterations, max_distance as float32, tolerance as float, init float64 [n, 4, 4] or None, grid_cells) of register,
    or ValueError."""
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or not 1 <= iterations < 2 ** 31:
        raise ValueError("register: iterations must be an integer >= 1")
    if max_distance is None:
        md = np.float32(np.inf)
    else:
        if isinstance(max_distance, bool) or not isinstance(max_distance, numbers.Real):
            raise ValueError("register: max_distance must be None or a number >= 0")
        with np.errstate(over="ignore"):
            md = np.float32(max_distance)
        if not md >= 0:
            raise ValueError("register: max_distance must be None or a number >= 0")
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real) or not float(tolerance) >= 0:
        raise ValueError("register: tolerance must be a number >= 0")
    if init is not None:
        try:
            init = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("register: init must be [4, 4] or [%d, 4, 4] finite numbers" % n)
        if init.shape == (4, 4):
            init = np.broadcast_to(init, (n, 4, 4))
        if init.shape != (n, 4, 4) or not np.isfinite(init).all():
            raise ValueError("register: init must be [4, 4] or [%d, 4, 4] finite numbers, got %s" % (n, init.shape))
        init = np.ascontiguousarray(init)
    return int(iterations), md, float(tolerance), init, _check_grid(grid, "register")


class PointBatch:
    """Point clouds packed and uploaded once, as MeshBatch does for meshes.  clouds: a list of points [P, 3] or of
    (points, normals [P, 3]) tuples.  estimate_normals: 0, or the k of estimate_normals(k) for clouds without normals."""

    def __init__(self, clouds, device=None, estimate_normals=0):
        p = pack_points(clouds)
        if estimate_normals != 0:
            _check_normals_k(estimate_normals)
            if p["normals"] is not None:
                raise ValueError("estimate_normals: the clouds already carry normals")
        self.device = _device(device)
        self.n = len(p["point_offsets"]) - 1
        self.point_offsets_host = p["point_offsets"]
        self.num_points = np.diff(p["point_offsets"])
        # one element at least: an empty tensor has no address to hand to the library
        pts = p["points"] if len(p["points"]) else np.zeros((1, 3), np.float32)
        self.points = torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        self.normals = None
        self.normal_status = None                                # host int32 [N] once estimate_normals has run
        self.clean_status = None                                 # host int32 [N] on the result of a cleaning call
        self.register_status = None                              # host int32 [N] on the result of register
        if p["normals"] is not None:
            nr = p["normals"] if len(p["normals"]) else np.zeros((1, 3), np.float32)
            self.normals = torch.from_numpy(np.ascontiguousarray(nr)).to(self.device)
        self.point_offsets = torch.from_numpy(p["point_offsets"]).to(self.device)
        if estimate_normals:
            self.estimate_normals(estimate_normals)

    def __len__(self):
        return self.n

    def group(self, a, b):
        """The C-ABI arguments of clouds [a, b): pointers into the packed arrays (no copy); the last is the grid-size
        hint (the largest cloud)."""
        po = self.point_offsets_host
        return (self.points.data_ptr() + int(po[a]) * 12, self.point_offsets.data_ptr() + a * 8, b - a,
                int(po[b] - po[a]), int(self.num_points[a:b].max()))

    def group_normals(self, a):
        """The normals pointer of the group that starts at cloud a (None without normals)."""
        return None if self.normals is None else self.normals.data_ptr() + int(self.point_offsets_host[a]) * 12

    @classmethod
    def from_device(cls, points, point_offsets_host, normals=None):
        """A batch from tensors that are on the device already, with no host round trip: points float32 [sum P, 3]
        (contiguous), point_offsets_host int64 [N + 1] on the host (from 0, non-decreasing, ending at sum P), normals
        float32 [sum P, 3] or None.  The points are not read: what pack_points checks on the host (finite values) is the
        device's per-cloud status here."""
        po = np.ascontiguousarray(np.asarray(point_offsets_host, dtype=np.int64))
        if po.ndim != 1 or len(po) < 2 or po[0] != 0 or (np.diff(po) < 0).any():
            raise ValueError("from_device: point_offsets must be [N + 1], start at 0 and not decrease")
        if np.diff(po).max() > MAX_POINTS:
            raise ValueError("from_device: a cloud has more than 2^24 points")
        for name, t in (("points", points), ("normals", normals)):
            if t is None and name == "normals":
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2
                    and t.shape[1] == 3 and t.is_contiguous() and t.shape[0] >= max(int(po[-1]), 1)):
                raise ValueError("from_device: %s must be a contiguous float32 device tensor [sum P, 3]" % name)
        if normals is not None and normals.device != points.device:
            raise ValueError("from_device: points and normals are on different devices")
        self = cls.__new__(cls)
        self.device = points.device
        self.n = len(po) - 1
        self.point_offsets_host = po
        self.num_points = np.diff(po)
        self.points = points
        self.normals = normals
        self.normal_status = None
        self.clean_status = None
        self.register_status = None
        self.point_offsets = torch.from_numpy(po).to(self.device)
        return self

    def register(self, target, iterations=30, max_distance=None, tolerance=0.0, init=None, grid=None, return_info=False,
                 return_correspondence=False):
        """Rigid registration on the device (contract: include/gvcnn_hip.h, "points in", registration): point-to-point
        ICP of cloud m of this batch (the source) onto cloud m of `target`, a PointBatch of the same length on the same
        device.  Every round matches each moved source point to its exact nearest target point (ties to the lower id),
        keeps the pairs within max_distance (None: all of them) and solves for the rigid motion of the original source
        onto its matches (Horn's quaternion); at most `iterations` rounds, a pair stops earlier once its rmse changes by
        no more than `tolerance` between two rounds (0: an exact fixed point only).  init: a [4, 4] or [N, 4, 4] float64
        starting transform (the identity without).  grid: as for estimate_normals, it changes the speed alone.  Returns
        a NEW batch of the moved source, normals rotated, normal_status carried along, with register_status host int32
        [N]: GV_RENDER_* of the pair (the source's, else the target's) with GV_POINTS_ICP_CONVERGED / _FEW_PAIRS /
        _NONFINITE or-ed in.  Only that status is read back.  Returns the batch, or (batch, transforms float64 [N, 4, 4],
        (rmse float64 [N], inliers int32 [N], rounds used int32 [N]) with return_info, correspondence int32 [sum P] (the
        matched target id of the last round, -1 for a rejected point) with return_correspondence), on the device."""
        if not isinstance(target, PointBatch):
            raise ValueError("register: target must be a PointBatch")
        if target.n != self.n:
            raise ValueError("register: %d source clouds but %d target clouds" % (self.n, target.n))
        if target.device != self.device:
            raise ValueError("register: source on %s but target on %s" % (self.device, target.device))
        iterations, md, tol, init, grid = _check_register_args(self.n, iterations, max_distance, tolerance, init, grid)
        lib = _lib.load()
        rows = self.points.shape[0]
        total_s, total_t = int(self.point_offsets_host[-1]), int(target.point_offsets_host[-1])
        with torch.cuda.device(self.device):
            ws, ws_bytes = self._workspace(lib, "gv_points_register_workspace_bytes", total_s, total_t, grid)
            transforms = torch.zeros((self.n, 4, 4), dtype=torch.float64, device=self.device)
            rmse = torch.zeros(self.n, dtype=torch.float64, device=self.device)
            inliers = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            used = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            corr = torch.full((rows,), -1, dtype=torch.int32, device=self.device) if return_correspondence else None
            moved = torch.zeros((rows, 3), dtype=torch.float32, device=self.device)
            moved_normals = None if self.normals is None else torch.zeros((rows, 3), dtype=torch.float32, device=self.device)
            status = torch.empty(self.n, dtype=torch.int32, device=self.device)
            s, t = self.group(0, self.n), target.group(0, self.n)
            rc = lib.gv_points_register(
                s[0], s[1], t[0], t[1], self.n, total_s, total_t, s[4], t[4], self.group_normals(0),
                None if init is None else init.ctypes.data, iterations, float(md), tol, grid, transforms.data_ptr(),
                rmse.data_ptr(), inliers.data_ptr(), used.data_ptr(), None if corr is None else corr.data_ptr(),
                moved.data_ptr(), None if moved_normals is None else moved_normals.data_ptr(), ws.data_ptr(), ws_bytes,
                status.data_ptr(), _model._st())
            _lib.check(rc, "gv_points_register")
            st = status.cpu().numpy()                            # (init, a host array, stays alive past its copy)
        new = PointBatch.from_device(moved, self.point_offsets_host, moved_normals)
        new.point_offsets = self.point_offsets
        new.normal_status = None if self.normal_status is None else self.normal_status.copy()
        new.register_status = st
        extras = ((transforms, (rmse, inliers, used)) if return_info else ()) + ((corr,) if return_correspondence else ())
        return (new,) + extras if extras else new

    @staticmethod
    def merged(*batches):
        """Pair by pair, the clouds of several batches as one: cloud m of the result is cloud m of the first batch followed
        by cloud m of the second, and so on (what register leaves to do before voxel_downsample removes the doubled
        points of the overlap).  The batches have the same length, are on the same device and are all with normals or
        all without.  The points never leave the device: one concatenation and one gather by an index built from the
        host offsets.  normal_status, clean_status and register_status are None on the result."""
        if not batches or not all(isinstance(b, PointBatch) for b in batches):
            raise ValueError("merged: one PointBatch at least, and PointBatches only")
        first = batches[0]
        for b in batches[1:]:
            if b.n != first.n:
                raise ValueError("merged: batches of %d and %d clouds" % (first.n, b.n))
            if b.device != first.device:
                raise ValueError("merged: batches on %s and %s" % (first.device, b.device))
            if (b.normals is None) != (first.normals is None):
                raise ValueError("merged: normals are all or none across the batches")
        base = np.concatenate([[0], np.cumsum([b.points.shape[0] for b in batches])])
        rows = [np.arange(b.point_offsets_host[m], b.point_offsets_host[m + 1], dtype=np.int64) + base[k]
                for m in range(first.n) for k, b in enumerate(batches)]
        po = np.zeros(first.n + 1, np.int64)
        po[1:] = np.cumsum(np.sum([b.num_points for b in batches], axis=0))
        if np.diff(po).max() > MAX_POINTS:
            raise ValueError("merged: a cloud has more than 2^24 points")
        index = np.concatenate(rows) if int(po[-1]) else np.zeros(1, np.int64)      # (one row at least, as everywhere)
        with torch.cuda.device(first.device):
            idx = torch.from_numpy(index).to(first.device)
            points = torch.cat([b.points for b in batches]).index_select(0, idx)
            normals = None if first.normals is None else torch.cat([b.normals for b in batches]).index_select(0, idx)
        return PointBatch.from_device(points, po, normals)

    def _compact(self, lib, keep, selected, index, status, ws, ws_bytes, with_normals):
        """gv_points_compact on a selection -> (new batch, out_index); only the counts are read back."""
        rows = self.points.shape[0]
        out_points = torch.zeros((rows, 3), dtype=torch.float32, device=self.device)
        out_normals = torch.zeros((rows, 3), dtype=torch.float32, device=self.device) if with_normals else None
        out_index = torch.zeros(rows, dtype=torch.int32, device=self.device)
        out_offsets = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
        counts = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        rc = lib.gv_points_compact(
            *self.group(0, self.n), keep.data_ptr(), None if selected is None else selected.data_ptr(),
            None if index is None else index.data_ptr(), self.group_normals(0) if with_normals else None,
            status.data_ptr(), out_points.data_ptr(), None if out_normals is None else out_normals.data_ptr(),
            out_index.data_ptr(), out_offsets.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, _model._st())
        _lib.check(rc, "gv_points_compact")
        po = np.zeros(self.n + 1, np.int64)
        po[1:] = np.cumsum(counts.cpu().numpy().astype(np.int64))        # (the workspace is not reused before this sync)
        new = PointBatch.from_device(out_points, po, out_normals)
        new.point_offsets = out_offsets
        return new, out_index

    def _workspace(self, lib, query, *sizes):
        """(workspace, its bytes) as the size query `query` of the library asks for this batch: (n, *sizes)."""
        ws_bytes = getattr(lib, query)(self.n, *sizes)
        _lib.check(ws_bytes if ws_bytes < 0 else 0, query)
        return torch.empty(ws_bytes, dtype=torch.uint8, device=self.device), ws_bytes

    def _clean_workspace(self, lib, grid):
        return self._workspace(lib, "gv_points_clean_workspace_bytes", int(self.point_offsets_host[-1]), grid)

    def remove_outliers(self, k=16, std_ratio=2.0, grid=None, return_index=False, return_stats=False):
        """Statistical outlier removal on the device (contract: include/gvcnn_hip.h, "points in", cleaning): a point
        goes when the mean distance to its k nearest neighbours (k: 1..32) exceeds the cloud's mean of that figure by
        more than std_ratio (>= 0) standard deviations.  Returns a NEW batch of the kept points in their order; normals
        and normal_status are carried along.  grid: as for estimate_normals, it changes the speed alone.  Sets
        clean_status on the result, host int32 [N]: GV_RENDER_* of the cloud, with GV_POINTS_CLEAN_PASSTHROUGH when it
        went through unchanged.  Only the counts are read back.  Returns the batch, or (batch, index int32 [new sum P]
        (ids within the original cloud), (mean_dist float32 [old sum P], stats float64 [N, 3] = mu, sigma, threshold),
        each on request), on the device."""
        k, ratio, grid = _check_outlier_args(k, std_ratio, grid)
        lib = _lib.load()
        rows = self.points.shape[0]
        with torch.cuda.device(self.device):
            ws, ws_bytes = self._clean_workspace(lib, grid)
            keep = torch.zeros(rows, dtype=torch.int32, device=self.device)
            md = torch.zeros(rows, dtype=torch.float32, device=self.device) if return_stats else None
            stats = torch.zeros((self.n, 3), dtype=torch.float64, device=self.device) if return_stats else None
            status = torch.empty(self.n, dtype=torch.int32, device=self.device)
            rc = lib.gv_points_outlier_select(
                *self.group(0, self.n), k, float(ratio), grid, keep.data_ptr(), None if md is None else md.data_ptr(),
                None if stats is None else stats.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(), _model._st())
            _lib.check(rc, "gv_points_outlier_select")
            new, index = self._compact(lib, keep, None, None, status, ws, ws_bytes, self.normals is not None)
            new.clean_status = status.cpu().numpy()
        new.normal_status = None if self.normal_status is None else self.normal_status.copy()
        extras = ((index,) if return_index else ()) + (((md, stats),) if return_stats else ())
        return (new,) + extras if extras else new

    def voxel_downsample(self, voxel, relative=False, return_index=False):
        """Voxel downsampling on the device (contract: include/gvcnn_hip.h, "points in", cleaning): one point per
        occupied voxel, the centroid of the voxel's points, in the order of each voxel's first point.  voxel: the edge
        length, a number or one number per cloud, in the clouds' units, or with relative=True as a fraction of the
        cloud's largest bounding-box extent.  Returns a NEW batch; a batch with normals gives each centroid the normal
        of the voxel's point nearest to it (normals are not averaged), and normal_status becomes None.  Sets
        clean_status on the result, host int32 [N], as remove_outliers does (GV_POINTS_CLEAN_PASSTHROUGH: a voxel size
        that is not > 0 on the device, or below 2^-21 of the extent).  Returns the batch, or (batch, index int32 [new
        sum P]: the id within the original cloud of that nearest point), on the device."""
        voxel, relative = _check_voxel_args(voxel, relative, self.n)
        lib = _lib.load()
        rows = self.points.shape[0]
        with torch.cuda.device(self.device):
            ws, ws_bytes = self._clean_workspace(lib, 0)
            keep = torch.zeros(rows, dtype=torch.int32, device=self.device)
            centroids = torch.zeros((rows, 3), dtype=torch.float32, device=self.device)
            index = torch.full((rows,), -1, dtype=torch.int32, device=self.device)
            status = torch.empty(self.n, dtype=torch.int32, device=self.device)
            rc = lib.gv_points_voxel_select(
                *self.group(0, self.n), voxel.ctypes.data, relative, 0, keep.data_ptr(), centroids.data_ptr(),
                index.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(), _model._st())
            _lib.check(rc, "gv_points_voxel_select")
            new, out_index = self._compact(lib, keep, centroids, index, status, ws, ws_bytes, self.normals is not None)
            new.clean_status = status.cpu().numpy()              # (voxel, a host array, stays alive past its copy)
        return (new, out_index) if return_index else new

    def estimate_normals(self, k=16, orient="outward", viewpoint=None, grid=None, return_neighbors=False,
                         return_variation=False):
        """Estimate every point's normal on the device from its k nearest neighbours within its cloud (contract:
        include/gvcnn_hip.h, "points in", normal estimation) and keep them as the batch's normals, replacing any it had.
        k: 3..32.  orient: "outward" (away from the centre of the cloud's bounding box), "viewpoint" (towards
        `viewpoint`, the sensor position, three numbers) or "none" (the largest component positive).  grid: cells per
        axis of the search grid, 1..128, or None for auto; it changes the speed alone.  Sets normal_status, host int32
        [N]: GV_RENDER_* of the cloud, with GV_POINTS_DEGENERATE_NORMAL or-ed in when some point's neighbourhood is
        coincident or collinear (that point's normal is (0, 0, 0): it takes the depth factor).  Returns the batch, or
        (batch, neighbors int32 [sum P, k] (ids within the cloud by rank, -1 past min(k, P)), variation float32 [sum P]
        (l0 / (l0 + l1 + l2)), each on request), on the device."""
        k, orient, viewpoint, grid = _check_normals_args(k, orient, viewpoint, grid)
        lib = _lib.load()
        rows = self.points.shape[0]                              # sum P (1 for a batch without points)
        total = int(self.point_offsets_host[-1])
        with torch.cuda.device(self.device):
            ws, ws_bytes = self._workspace(lib, "gv_points_normals_workspace_bytes", total, grid)
            normals = torch.zeros((rows, 3), dtype=torch.float32, device=self.device)
            nb = torch.full((rows, k), -1, dtype=torch.int32, device=self.device) if return_neighbors else None
            var = torch.zeros(rows, dtype=torch.float32, device=self.device) if return_variation else None
            status = torch.empty(self.n, dtype=torch.int32, device=self.device)
            rc = lib.gv_points_estimate_normals(
                *self.group(0, self.n), k, orient, None if viewpoint is None else viewpoint.ctypes.data, grid,
                normals.data_ptr(), None if nb is None else nb.data_ptr(), None if var is None else var.data_ptr(),
                ws.data_ptr(), ws_bytes, status.data_ptr(), _model._st())
            _lib.check(rc, "gv_points_estimate_normals")
            self.normal_status = status.cpu().numpy()            # (the workspace is not reused before this sync)
        self.normals = normals
        extras = tuple(x for x in (nb, var) if x is not None)
        return (self,) + extras if extras else self


def estimate_normals(points, k=16, orient="outward", viewpoint=None, grid=None, device=None):
    """The estimated normals float32 [P, 3] of one host cloud points [P, 3]: PointBatch([points]).estimate_normals(...),
    copied back."""
    _check_normals_args(k, orient, viewpoint, grid)
    batch = PointBatch([points], device).estimate_normals(k, orient, viewpoint, grid)
    return batch.normals.cpu().numpy()[:int(batch.num_points[0])]


def _kept(batch, index):
    n = int(batch.num_points[0])
    return batch.points.cpu().numpy()[:n], index.cpu().numpy()[:n]


def remove_outliers(points, k=16, std_ratio=2.0, grid=None, device=None):
    """(kept points float32 [P', 3], index int32 [P'] into `points`) of one host cloud points [P, 3]:
    PointBatch([points]).remove_outliers(...), copied back."""
    _check_outlier_args(k, std_ratio, grid)
    return _kept(*PointBatch([points], device).remove_outliers(k, std_ratio, grid, return_index=True))


def voxel_downsample(points, voxel, relative=False, device=None):
    """(centroids float32 [P', 3], index int32 [P']: the point of `points` nearest to each centroid within its voxel) of
    one host cloud points [P, 3]: PointBatch([points]).voxel_downsample(...), copied back."""
    _check_voxel_args(voxel, relative, 1)
    return _kept(*PointBatch([points], device).voxel_downsample(voxel, relative, return_index=True))


def register(source, target, iterations=30, max_distance=None, tolerance=0.0, init=None, grid=None, device=None):
    """(moved points float32 [P, 3], transform float64 [4, 4]) of one host pair: source [P, 3] registered onto target
    [Q, 3]: PointBatch([source]).register(PointBatch([target]), ...), copied back."""
    _check_register_args(1, iterations, max_distance, tolerance, init, grid)
    batch, transforms, _ = PointBatch([source], device).register(PointBatch([target], device), iterations, max_distance,
                                                                 tolerance, init, grid, return_info=True)
    return batch.points.cpu().numpy()[:int(batch.num_points[0])], transforms.cpu().numpy()[0]


def random_rotations(n, mode="z", seed=0):
    """[n, 3, 3] float32 rotation matrices, built in float64 from np.random.RandomState(seed) and rounded once.
    mode 'z': about the up axis by a uniform angle; 'so3': uniform over all rotations (unit quaternions)."""
    rng = np.random.RandomState(seed)
    if mode == "z":
        a = rng.uniform(0.0, 2.0 * np.pi, size=n)
        c, s = np.cos(a), np.sin(a)
        R = np.zeros((n, 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, -s, s, c, 1.0
    elif mode == "so3":
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                      2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                      2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    else:
        raise ValueError("mode must be 'z' or 'so3', not %r" % (mode,))
    return R.astype(np.float32)


def icosphere(subdivisions=0):
    """(verts, tris) of the unit icosphere: 20 * 4^subdivisions outward-wound faces (synthetic test and benchmark
    meshes)."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(verts, np.float32), np.array(f, np.int32)


def default_azimuths(num_views):
    """a_i = (i + 1) * 360 / V: obj2png.py's azim * (i + 1) (V = 8, azim = 45)."""
    return [(i + 1) * 360.0 / num_views for i in range(num_views)]


def camera_matrices(elevation, azimuths):
    """[V, 3, 3] float32: rows right, up, forward (eye -> origin) of matplotlib's view_init(elev, azim), +z up."""
    return _camera_matrices64(elevation, azimuths).astype(np.float32)


def _camera_matrices64(elevation, azimuths):
    azimuths = list(azimuths)
    el = np.broadcast_to(np.asarray(elevation, np.float64), (len(azimuths),))
    C = np.zeros((len(azimuths), 3, 3))
    for i, (e, a) in enumerate(zip(el, azimuths)):
        e, a = math.radians(float(e)), math.radians(float(a))
        eye = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
        f = -eye
        r = np.array([-math.sin(a), math.cos(a), 0.0])
        u = np.cross(r, f)
        C[i] = np.stack([r, u, f])
    return C


def shading_vectors(elevation, azimuths, light):
    """(lights, halfs) float32 [V, 3] of smooth shading, built in float64 and rounded once.  light: a direction
    (normalised here) or "camera", the headlight: the unit vector from the origin towards every view's eye (the negated
    forward row of its camera).  halfs: m_v = normalize(l_v + eye_v), the Blinn half-vector of a directional viewer
    (zero where the light looks straight back at the eye)."""
    eye = -_camera_matrices64(elevation, azimuths)[:, 2, :]
    if isinstance(light, str):
        lights = eye.copy()
    else:
        lt = np.asarray(light, np.float64)
        lights = np.broadcast_to(lt / np.linalg.norm(lt), eye.shape)
    m = lights + eye
    nm = np.linalg.norm(m, axis=1, keepdims=True)
    halfs = np.where(nm > 0, m / np.where(nm > 0, nm, 1.0), 0.0)
    # (C order spelled out: astype keeps a broadcast array's stride order, and the kernels read [V, 3] rows)
    return np.ascontiguousarray(lights, dtype=np.float32), np.ascontiguousarray(halfs, dtype=np.float32)


def projection(height, width, fov):
    """(flags bit, proj_scale, persp_dist, depth_a, depth_b) in float64 (the descriptor rounds them to fp32)."""
    half = min(height, width) / 2.0
    if fov == 0:
        return 0, half, 0.0, 0.0, 0.0
    t = math.radians(fov) / 2.0
    D = 1.0 / math.sin(t)
    return _lib.GV_RENDER_PERSPECTIVE, half / math.tan(t), D, (D + 1.0) / 2.0, (D * D - 1.0) / 2.0


def _check_reflection(diffuse, specular, shininess, light):
    """The reflection keywords of ViewRenderer (and of its point_reflection), each on its own."""
    if diffuse not in ("wrap", "lambert"):
        raise ValueError("diffuse must be 'wrap' or 'lambert'")
    if isinstance(light, str) and light != "camera":
        raise ValueError("light must be a nonzero 3-vector or 'camera'")
    if isinstance(specular, bool) or not isinstance(specular, numbers.Real) or not 0.0 <= specular <= 1.0:
        raise ValueError("specular must be in [0, 1]")
    if (isinstance(shininess, bool) or not isinstance(shininess, numbers.Integral)
            or shininess not in (1, 2, 4, 8, 16, 32, 64, 128)):
        raise ValueError("shininess must be one of 1, 2, 4, ..., 128")


def _unit_light(light):
    lt = np.asarray(light, np.float64)
    if lt.shape != (3,) or not np.isfinite(lt).all() or not np.linalg.norm(lt) > 0:
        raise ValueError("light must be a nonzero 3-vector")
    return lt / np.linalg.norm(lt)


def _shading_desc(diffuse, specular, shininess):
    sh = _lib.RenderShading()
    sh.flags = _lib.GV_RENDER_LAMBERT if diffuse == "lambert" else 0
    sh.shininess, sh.specular = int(shininess), float(specular)
    return sh


class _MeshKind:
    """What ViewRenderer._draw_group calls to draw meshes: gv_render_* (csrc/render.hip).  args: the batch's group(a, b);
    ws_args: the five arguments from the descriptor to the workspace size, which every call takes after args."""
    batch, prefix = MeshBatch, "gv_render"

    def __init__(self, r):
        self.r, self.desc, self.samples = r, r.desc, r.samples

    def workspace_bytes(self, args):
        """(workspace bytes, what else counts against the cap: the normal table of a smooth render)."""
        r = self.r
        ws_bytes = r.lib.gv_render_workspace_bytes(args[4], r.V, r.H, r.W, args[6])
        _lib.check(ws_bytes if ws_bytes < 0 else 0, "gv_render_workspace_bytes")
        nb = 0
        if r.shading == "smooth":
            nb = r.lib.gv_render_normals_bytes(r.V, r.desc.flags, args[5])
            _lib.check(nb if nb < 0 else 0, "gv_render_normals_bytes")
        return ws_bytes, nb

    def prepare(self, args, a, b, ws_args, info):
        r = self.r
        if not r._ss:
            return r.lib.gv_render_prepare(*args, *ws_args, *info, _model._st())
        return r.lib.gv_render_prepare_ss(*args, *ws_args, *info, r.samples, _model._st())

    def draw(self, batch, args, a, b, ws_args, out_args, nb):
        r = self.r
        if r.shading == "smooth":
            normals = torch.empty(nb, dtype=torch.uint8, device=r.device)
            rc = r.lib.gv_render_vertex_normals(*args, *ws_args, *batch.group_adjacency(a, b), normals.data_ptr(), nb,
                                                _model._st())
            _lib.check(rc, "gv_render_vertex_normals")
            return r.lib.gv_render_draw_smooth(*args, *ws_args, *out_args, r.samples, r.shade_desc, r.lights.data_ptr(),
                                               r.halfs.data_ptr(), normals.data_ptr(), nb, _model._st())
        if not r._ss:
            return r.lib.gv_render_draw(*args, *ws_args, *out_args, _model._st())
        return r.lib.gv_render_draw_ss(*args, *ws_args, *out_args, r.samples, _model._st())


class _PointKind:
    """... and to splat point clouds: gv_points_* (csrc/render_points.hip), one sample per pixel.  radii: float32 [N] on
    the host; normal: shading="normal"."""
    batch, prefix = PointBatch, "gv_points"

    def __init__(self, r, radii, normal):
        self.r, self.desc, self.samples, self.radii, self.normal = r, r.point_desc, 1, radii, normal

    def workspace_bytes(self, args):
        r = self.r
        ws_bytes = r.lib.gv_points_workspace_bytes(args[2], r.V, r.H, r.W)
        _lib.check(ws_bytes if ws_bytes < 0 else 0, "gv_points_workspace_bytes")
        return ws_bytes, 0

    def prepare(self, args, a, b, ws_args, info):
        rad = self.radii[a:b]                                            # host memory: self.radii outlives the call
        return self.r.lib.gv_points_prepare(*args, rad.ctypes.data, *ws_args, *info, _model._st())

    def draw(self, batch, args, a, b, ws_args, out_args, extra):
        r, shade = self.r, (None, None, None, None)
        if self.normal:
            if r._point_vectors is None:
                r._point_vectors = (torch.from_numpy(r.point_lights_host).to(r.device),
                                    torch.from_numpy(r.point_halfs_host).to(r.device))
            shade = (batch.group_normals(a), r.point_shade_desc, r._point_vectors[0].data_ptr(),
                     r._point_vectors[1].data_ptr())
        return r.lib.gv_points_draw(*args, *ws_args, *out_args, *shade, _model._st())


class ViewRenderer:
    """V views of H x W per mesh (rendering contract: the module docstring).  elevation: degrees, one for all views or
    one per view; azimuths: degrees (default (i + 1) * 360 / V); fov: 0 (orthographic) or a perspective field of view
    in degrees, (0, 120]; fit: the normalised radius in (0, 1]; color / background: RGB in [0, 1]; light: a direction
    (normalised here); max_workspace_bytes: a batch whose workspace or tile lists would pass it is rendered in groups of
    meshes, with identical results; samples: 1, 2 or 4 coverage samples per pixel and axis (anti-aliasing; 1 is one sample
    at the pixel centre); shading: "flat" (one factor per triangle) or "smooth" (Phong reflection on interpolated vertex
    normals, per sample).  Smooth only: light="camera" (a headlight that travels with the view), diffuse="lambert"
    (max(s, 0); "wrap" is matplotlib's (s + 1) / 2; two_sided makes both |s|), specular in [0, 1] with shininess 1, 2,
    4, ..., 128 (the exponent of the highlight).  point_reflection: a dict with any of diffuse, specular, shininess, light,
    two_sided for render_points(shading="normal") alone (it may hold what a flat mesh renderer refuses); without it the
    splatter reflects as the renderer does."""

    def __init__(self, num_views, height, width, elevation=30.0, azimuths=None, fov=0.0, fit=0.9,
                 color=DEFAULT_COLOR, background=DEFAULT_BACKGROUND, light=DEFAULT_LIGHT, ambient=0.3,
                 two_sided=False, device=None, max_workspace_bytes=DEFAULT_MAX_WORKSPACE, samples=1, shading="flat",
                 diffuse="wrap", specular=0.0, shininess=16, point_reflection=None):
        if not 1 <= int(num_views) <= MAX_VIEWS:
            raise ValueError("num_views must be in [1, %d]" % MAX_VIEWS)
        if not (1 <= int(height) <= MAX_SIDE and 1 <= int(width) <= MAX_SIDE):
            raise ValueError("height and width must be in [1, %d]" % MAX_SIDE)
        if not 0.0 < fit <= 1.0:
            raise ValueError("fit must be in (0, 1]")
        if not 0.0 <= ambient <= 1.0:
            raise ValueError("ambient must be in [0, 1]")
        if not (fov == 0 or 0.0 < fov <= 120.0):
            raise ValueError("fov must be 0 (orthographic) or in (0, 120] degrees")
        if samples not in (1, 2, 4):
            raise ValueError("samples must be 1, 2 or 4")
        if shading not in ("flat", "smooth"):
            raise ValueError("shading must be 'flat' or 'smooth'")
        _check_reflection(diffuse, specular, shininess, light)
        # render_points(shading="normal") reflects as the renderer does, or as point_reflection says: a dict with any of
        # diffuse, specular, shininess, light, two_sided (so a flat mesh renderer can still splat with a headlight)
        pr = {"diffuse": diffuse, "specular": specular, "shininess": shininess, "light": light, "two_sided": two_sided}
        if point_reflection is not None:
            if not isinstance(point_reflection, dict) or set(point_reflection) - set(pr):
                raise ValueError("point_reflection is a dict with keys among %s" % sorted(pr))
            pr.update(point_reflection)
            _check_reflection(pr["diffuse"], pr["specular"], pr["shininess"], pr["light"])
        if shading == "flat":
            # the flat table is per triangle and view-independent, and stays so
            for bad, what in ((isinstance(light, str), "light='camera'"), (diffuse != "wrap", "diffuse='lambert'"),
                              (specular != 0, "a specular term"), (shininess != 16, "a shininess")):
                if bad:
                    raise ValueError("%s needs shading='smooth'" % what)
        self.samples = int(samples)
        self._ss = self.samples > 1                      # through gv_render_*_ss (samples = 1: the original pair)
        self.shading, self.diffuse, self.specular, self.shininess = shading, diffuse, float(specular), int(shininess)
        self.light_mode = "camera" if isinstance(light, str) else "world"
        if self.light_mode == "camera":
            light = DEFAULT_LIGHT                        # the flat table (a smooth sample's fallback) keeps a world light
        self.lib = _lib.load()
        self.V, self.H, self.W = int(num_views), int(height), int(width)
        self.azimuths = default_azimuths(self.V) if azimuths is None else [float(a) for a in azimuths]
        if len(self.azimuths) != self.V:
            raise ValueError("azimuths must hold num_views values")
        self.elevation = elevation
        self.device = _device(device)
        self.cameras_host = camera_matrices(elevation, self.azimuths)
        lt = _unit_light(light)
        flags, k, D, a, b = projection(self.H, self.W, fov)
        d = _lib.RenderDesc()
        d.height, d.width, d.num_views = self.H, self.W, self.V
        d.flags = flags | (_lib.GV_RENDER_TWO_SIDED if two_sided else 0)
        d.fit, d.proj_scale, d.persp_dist, d.depth_a, d.depth_b, d.ambient = fit, k, D, a, b, ambient
        for dst, src in ((d.light, lt), (d.color, color), (d.background, background)):
            src = np.asarray(src, np.float64)
            if src.shape != (3,) or not np.isfinite(src).all():
                raise ValueError("color, background and light are RGB / xyz triples")
            for i in range(3):
                dst[i] = float(src[i])
        self.desc = d
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.cameras = torch.from_numpy(self.cameras_host).to(self.device)
        self.status = None
        self.lights_host, self.halfs_host = shading_vectors(elevation, self.azimuths,
                                                            "camera" if self.light_mode == "camera" else lt)
        if shading == "smooth":
            self.shade_desc = _shading_desc(diffuse, specular, shininess)
            self.lights = torch.from_numpy(self.lights_host).to(self.device)
            self.halfs = torch.from_numpy(self.halfs_host).to(self.device)
        # the point splatter's reflection: its own descriptor copy (two_sided), shading descriptor, lights and halfs
        self.point = pr
        self.point_desc = _lib.RenderDesc.from_buffer_copy(d)
        self.point_desc.flags = flags | (_lib.GV_RENDER_TWO_SIDED if pr["two_sided"] else 0)
        self.point_shade_desc = _shading_desc(pr["diffuse"], pr["specular"], pr["shininess"])
        self.point_lights_host, self.point_halfs_host = shading_vectors(
            elevation, self.azimuths, "camera" if isinstance(pr["light"], str) else _unit_light(pr["light"]))
        self._point_vectors = None                       # (lights, halfs) on the device, on the first "normal" render

    def point_descriptor(self):
        """descriptor() with the reflection fields render_points(shading="normal") uses, for an oracle."""
        d = self.descriptor()
        d.update({"flags": self.point_desc.flags, "diffuse": self.point["diffuse"],
                  "light_mode": "camera" if isinstance(self.point["light"], str) else "world",
                  "specular": float(np.float32(self.point["specular"])), "shininess": int(self.point["shininess"]),
                  "lights": self.point_lights_host.copy(), "halfs": self.point_halfs_host.copy()})
        return d

    def descriptor(self):
        """The descriptor's fields as Python values (fp32-rounded), for an oracle."""
        d = self.desc
        return {"height": d.height, "width": d.width, "num_views": d.num_views, "flags": d.flags, "fit": d.fit,
                "proj_scale": d.proj_scale, "persp_dist": d.persp_dist, "depth_a": d.depth_a, "depth_b": d.depth_b,
                "ambient": d.ambient, "light": list(d.light), "color": list(d.color),
                "background": list(d.background), "cameras": self.cameras_host.copy(), "samples": self.samples,
                "shading": self.shading, "diffuse": self.diffuse, "light_mode": self.light_mode,
                "specular": float(np.float32(self.specular)), "shininess": self.shininess,
                "lights": self.lights_host.copy(), "halfs": self.halfs_host.copy()}

    def _rotations(self, rotations, n):
        if rotations is None:
            return None
        return torch.from_numpy(check_rotations(rotations, n)).to(self.device)

    def _batch(self, cls, batch):
        """batch as a MeshBatch / PointBatch (cls) on the renderer's device."""
        if not isinstance(batch, cls):
            batch = cls(batch, self.device)
        elif batch.device != self.device:
            raise ValueError("the batch lives on %s, the renderer on %s" % (batch.device, self.device))
        return batch

    def _draw_group(self, kind, batch, a, b, rot, output, out, ids, depth, status):
        """Render shapes [a, b) into out[a:b] (and the buffers); halves the group when its workspace or its tile lists
        would pass the workspace cap.  kind: _MeshKind or _PointKind."""
        lib, n = self.lib, b - a
        args = batch.group(a, b)

        def halves():
            h = (a + b) // 2
            self._draw_group(kind, batch, a, h, rot, output, out, ids, depth, status)
            self._draw_group(kind, batch, h, b, rot, output, out, ids, depth, status)
        ws_bytes, extra = kind.workspace_bytes(args)
        if ws_bytes + extra > self.max_workspace_bytes and n > 1:
            return halves()
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        info = torch.empty(1 + (n + 1) // 2, dtype=torch.int64, device=self.device)     # pair total, then status
        st_dev = info[1:].view(torch.int32)
        rp = None if rot is None else rot.data_ptr() + a * 36
        ws_args = (kind.desc, self.cameras.data_ptr(), rp, ws.data_ptr(), ws_bytes)
        rc = kind.prepare(args, a, b, ws_args, (info.data_ptr(), st_dev.data_ptr()))
        _lib.check(rc, kind.prefix + "_prepare")
        host = info.cpu().numpy()                                        # the one host read of a render
        total = int(host[0])
        status[a:b] = host[1:].view(np.int32)[:n]
        bins_bytes = lib.gv_render_bins_bytes(total)
        _lib.check(bins_bytes if bins_bytes < 0 else 0, "gv_render_bins_bytes")
        if ws_bytes + extra + bins_bytes > self.max_workspace_bytes and n > 1:
            del ws, info
            return halves()
        bins = torch.empty(bins_bytes, dtype=torch.uint8, device=self.device)
        img = self.V * self.H * self.W
        esz = 1 if output == _lib.GV_RENDER_OUT_U8 else 4
        grid = img * kind.samples ** 2 * 4                               # ids and depth: one entry per sample
        out_args = (bins.data_ptr(), bins_bytes, total, output, out.data_ptr() + a * img * 3 * esz,
                    None if ids is None else ids.data_ptr() + a * grid,
                    None if depth is None else depth.data_ptr() + a * grid)
        _lib.check(kind.draw(batch, args, a, b, ws_args, out_args, extra), kind.prefix + "_draw")

    def _render(self, batch, rotations, out, output, return_buffers, kind=None):
        """The body of every render call; kind: a _PointKind for render_points (default: meshes)."""
        kind = kind or _MeshKind(self)
        with torch.cuda.device(self.device):
            batch = self._batch(kind.batch, batch)
            n = batch.n
            rot = self._rotations(rotations, n)
            shape = (n, self.V, self.H, self.W, 3)
            dt = torch.uint8 if output == _lib.GV_RENDER_OUT_U8 else torch.float32
            if out is None:
                out = torch.empty(shape, dtype=dt, device=self.device)
            elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != dt or not out.is_contiguous()
                  or _device(out.device) != self.device):
                raise ValueError("out must be a contiguous %s tensor %s on %s" % (dt, shape, self.device))
            face_id = depth = None
            if return_buffers:
                grid = (n, self.V, self.samples * self.H, self.samples * self.W)        # one entry per sample
                face_id = torch.empty(grid, dtype=torch.int32, device=self.device)
                depth = torch.empty(grid, dtype=torch.int32, device=self.device)        # uint32 bits
            status = np.zeros(n, np.int32)
            self._draw_group(kind, batch, 0, n, rot, output, out, face_id, depth, status)
            self.status = status
            if return_buffers:
                return out, face_id, depth
            return out

    # -- points in (csrc/render_points.hip; contract: include/gvcnn_hip.h, "points in") ---------------------------------
    def _point_radii(self, batch, radius):
        """radius -> float32 [N] in normalised units: "auto" (auto_point_radius per cloud), one positive number, or one
        per cloud."""
        n = batch.n
        if isinstance(radius, str):
            if radius != "auto":
                raise ValueError("radius must be 'auto', a positive number or one per cloud")
            r = [auto_point_radius(p, self.desc.fit, self.desc.proj_scale) for p in batch.num_points]
            return np.ascontiguousarray(r, dtype=np.float32)
        try:
            r = np.asarray(radius, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("radius must be 'auto', a positive number or one per cloud")
        if isinstance(radius, bool) or r.dtype == bool or (r.ndim != 0 and r.shape != (n,)):
            raise ValueError("radius must be 'auto', a positive number or one per cloud (%d)" % n)
        r = np.ascontiguousarray(np.broadcast_to(r, (n,)), dtype=np.float32)
        if not (np.isfinite(r).all() and (r > 0).all()):
            raise ValueError("radius must be finite and positive in fp32")
        return r

    def _render_points(self, batch, rotations, out, output, return_buffers, radius, shading):
        if self.samples != 1:
            raise ValueError("render_points draws one sample per pixel: the renderer has samples=%d" % self.samples)
        if shading not in ("depth", "normal"):
            raise ValueError("shading must be 'depth' or 'normal'")
        batch = self._batch(PointBatch, batch)
        if shading == "normal" and batch.normals is None:
            raise ValueError("shading='normal' needs a batch with normals")
        kind = _PointKind(self, self._point_radii(batch, radius), shading == "normal")
        return self._render(batch, rotations, out, output, return_buffers, kind)

    def render_points(self, batch, rotations=None, out=None, quantize=True, return_buffers=False, radius="auto",
                      shading="depth"):
        """views fp32 [N, V, H, W, 3] of N point clouds splatted as screen-parallel discs (and (point_id int32, depth)
        [N, V, H, W] with return_buffers, as render returns face_id and depth).  batch: a PointBatch or a list of points
        [P, 3] / (points, normals) tuples.  radius: the disc's radius in normalised units (the unit sphere has radius 1;
        one pixel is 1 / proj_scale): a positive number, one per cloud, or "auto" (auto_point_radius).  shading:
        "depth" (nearer is brighter: f = ambient + (1 - ambient) * (1 - depth)) or "normal" (the reflection model of
        shading="smooth" on the points' normals, with this renderer's diffuse / specular / shininess / light /
        two_sided or its point_reflection).  The renderer must have samples=1.  Sets `status` as render does."""
        output = _lib.GV_RENDER_OUT_F32_QUANTIZED if quantize else _lib.GV_RENDER_OUT_F32
        return self._render_points(batch, rotations, out, output, return_buffers, radius, shading)

    def render_points_uint8(self, batch, rotations=None, out=None, return_buffers=False, radius="auto", shading="depth"):
        """render_points as uint8 [N, V, H, W, 3] on the device (what a PNG of the render holds)."""
        return self._render_points(batch, rotations, out, _lib.GV_RENDER_OUT_U8, return_buffers, radius, shading)

    def render_points_png(self, batch, rotations=None, filter="adaptive", color="auto", radius="auto", shading="depth"):
        """One list of V PNG files (bytes) per cloud: render_points_uint8, then the device encoder, as render_png."""
        return self._encode_png(self.render_points_uint8(batch, rotations, radius=radius, shading=shading), filter, color)

    def render(self, batch, rotations=None, out=None, quantize=True, return_buffers=False):
        """views fp32 [N, V, H, W, 3] on the device (and (face_id int32, depth) [N, V, S*H, S*W] with return_buffers, one
        entry per sample, S = samples; depth is an int32 tensor holding the uint32 values, -1 = 0xFFFFFFFF =
        background).  batch: a MeshBatch or a list of (verts, tris).  rotations: [N, 3, 3] rotation matrices
        (check_rotations) or None; pass them as a host array to keep to one host read (the tile-list size) per mesh
        group."""
        output = _lib.GV_RENDER_OUT_F32_QUANTIZED if quantize else _lib.GV_RENDER_OUT_F32
        return self._render(batch, rotations, out, output, return_buffers)

    def render_uint8(self, batch, rotations=None, out=None, return_buffers=False):
        """views uint8 [N, V, H, W, 3] on the device (what a PNG of the render holds)."""
        return self._render(batch, rotations, out, _lib.GV_RENDER_OUT_U8, return_buffers)

    def render_png(self, batch, rotations=None, filter="adaptive", color="auto"):
        """One list of V PNG files (bytes) per mesh: render_uint8, then the device encoder (records.encode_png_batch:
        the pixels stay on the device, the finished zlib streams come back).  Sets `status` as render_uint8 does."""
        return self._encode_png(self.render_uint8(batch, rotations), filter, color)

    def _encode_png(self, views, filter, color):
        from . import records
        n = views.shape[0]
        with torch.cuda.device(self.device):
            pngs = records.encode_png_batch(views.view(n * self.V, self.H, self.W, 3), filter, color)
        return [pngs[i * self.V:(i + 1) * self.V] for i in range(n)]
