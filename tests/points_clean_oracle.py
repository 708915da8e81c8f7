"""numpy restatement of the cleaning contract (include/gvcnn_hip.h, "points in", cleaning): a brute-force key table over
j != i, fp64 means in rank order, the tree sum as b[0::2] + b[1::2], voxel keys from a true fp32 division, centroids
through np.rint and int64 np.add.at, np.frexp for the exponent, the compaction as boolean indexing.  No grid and no hash
table: this is the answer the device's grid, table and schedule must not change."""
import numpy as np

F = np.float32
OK, EMPTY, NONFINITE, TOO_LARGE, BAD_OFFSETS = 0, 1, 3, 4, 5      # GV_RENDER_*
PASSTHROUGH = 0x200                                                # GV_POINTS_CLEAN_PASSTHROUGH
MIN_K, MAX_K = 1, 32
CHUNK = 512
TOO_FINE = np.float32(2097152.0)


# ---- statistical outlier selection ------------------------------------------------------------------------------------
def key_table(points, k):
    """keys uint64 [P, k_eff] of the k_eff = min(k, P - 1) smallest keys (bits(d2) << 32 | j) over j != i per point, in
    ascending order."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(p)
    keff = min(k, P - 1)
    out = np.zeros((P, max(keff, 0)), np.uint64)
    if keff <= 0:
        return out
    ids = np.arange(P, dtype=np.uint64)
    for a in range(0, P, CHUNK):
        q = p[a:a + CHUNK]
        with np.errstate(over="ignore"):
            dx = p[None, :, 0] - q[:, None, 0]                     # float32 throughout: one rounding per step
            dy = p[None, :, 1] - q[:, None, 1]
            dz = p[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]
        rows = np.arange(len(q))
        keys[rows, a + rows] = np.uint64(0xFFFFFFFFFFFFFFFF)       # j != i
        if keff < P:
            keys = np.partition(keys, keff - 1, axis=1)[:, :keff]
        out[a:a + CHUNK] = np.sort(keys, axis=1)
    return out


def line_cloud(P, seed):
    """(points float32 [P, 3], perm): P points on the x axis whose k = 1 key table costs O(P) (line_key_table), for clouds
    too large for key_table.  x: the cumulative sum of integer gaps in [1, 64) times 2^-8, exact in fp32 up to 2^24; the ids
    are a random permutation of the line order: id t holds the perm[t]-th point of the line."""
    rng = np.random.RandomState(seed)
    steps = np.cumsum(rng.randint(1, 64, size=P).astype(np.int64))
    assert steps[-1] < 1 << 24
    perm = rng.permutation(P)
    pts = np.zeros((P, 3), np.float32)
    pts[:, 0] = (steps[perm].astype(np.float64) / 256.0).astype(np.float32)
    return pts, perm


def line_key_table(points, perm):
    """key_table(points, 1) of a line_cloud from the two line neighbours of each point: a gap is at most 63 / 256, so d2 is
    exact in fp32 and grows strictly with the distance along the line; a tie between the two goes to the lower id, as the
    smaller key."""
    x = np.ascontiguousarray(points, dtype=np.float32)[:, 0]
    P = len(x)
    ids = np.empty(P, np.int64)
    ids[perm] = np.arange(P)                                       # ids[s]: the id of the s-th point of the line
    xs = x[ids]
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    side = []
    for nb, at in ((slice(0, P - 1), slice(1, P)), (slice(1, P), slice(0, P - 1))):    # the left, then the right neighbour
        dx = xs[nb] - xs[at]
        d2 = (dx * dx + np.float32(0.0)) + np.float32(0.0)
        assert d2.dtype == np.float32
        keys = np.full(P, none, np.uint64)
        keys[at] = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[nb].astype(np.uint64)
        side.append(keys)
    out = np.empty((P, 1), np.uint64)
    out[ids, 0] = np.minimum(side[0], side[1])
    return out


def mean_distances(keys):
    """m_i float64 [P]: (sqrt((double)d2_0) + ... ) / k_eff from 0.0, left to right in rank order."""
    P, keff = keys.shape
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    s = np.zeros(P, np.float64)
    for r in range(keff):
        s = s + np.sqrt(d2[:, r])
    return s / np.float64(keff)


def tree_sum(a):
    """T(a): pad with +0.0 to the next power of two, then b_t = a_2t + a_2t+1 level by level."""
    a = np.asarray(a, np.float64)
    n = 1
    while n < len(a):
        n *= 2
    b = np.zeros(n, np.float64)
    b[:len(a)] = a
    while len(b) > 1:
        b = b[0::2] + b[1::2]
    return np.float64(b[0])


def finite_cloud(p32):
    with np.errstate(over="ignore", invalid="ignore"):
        ext = p32.max(axis=0) - p32.min(axis=0)
    return bool(np.isfinite(p32).all() and np.isfinite(ext).all())


def outlier_select_cloud(points, k, std_ratio, keys=None):
    """One cloud: dict keep int32 [P], mean_dist float32 [P], stats float64 [3], status int.  keys: key_table(points, k')
    for some k' >= k, when the caller has it (the k smallest keys are a prefix)."""
    assert MIN_K <= k <= MAX_K and np.isfinite(std_ratio) and std_ratio >= 0
    p32 = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(p32)
    out = {"keep": np.ones(P, np.int32), "mean_dist": np.zeros(P, np.float32), "stats": np.zeros(3, np.float64),
           "status": OK}
    if P == 0:
        out["status"] = EMPTY
        return out
    if not finite_cloud(p32):
        out["status"] = NONFINITE | PASSTHROUGH
        return out
    if P < 2:
        return out
    keff = min(k, P - 1)
    keys = key_table(p32, k) if keys is None else keys[:, :keff]
    m = mean_distances(keys)
    mu = tree_sum(m) / np.float64(P)
    e = m - mu
    sigma = np.sqrt(tree_sum(e * e) / np.float64(P - 1))
    T = mu + np.float64(np.float32(std_ratio)) * sigma
    out["keep"] = (m <= T).astype(np.int32)
    out["mean_dist"] = m.astype(np.float32)
    out["stats"] = np.array([mu, sigma, T], np.float64)
    return out


# ---- voxel selection --------------------------------------------------------------------------------------------------
def voxel_select_cloud(points, voxel, relative):
    """One cloud: dict keep int32 [P], centroids float32 [P, 3], index int32 [P], status int, and for the tests keys
    uint64 [P] (each point's voxel key; None on a passthrough), h and centroids64 (the centroids before their one
    rounding to fp32)."""
    p32 = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(p32)
    out = {"keep": np.ones(P, np.int32), "centroids": p32.copy(), "index": np.arange(P, dtype=np.int32), "status": OK,
           "keys": None, "h": None}
    if P == 0:
        out["status"] = EMPTY
        return out
    if not finite_cloud(p32):
        out["status"] = NONFINITE | PASSTHROUGH
        return out
    mn = p32.min(axis=0)
    ext = p32.max(axis=0) - mn                                     # float32
    big = ext.max()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        h = np.float32(voxel) * big if relative else np.float32(voxel)
        assert h.dtype == np.float32
        bad = not (h > 0 and np.isfinite(h))
        if not bad:
            bad = bool(((ext / h) >= TOO_FINE).any())
    out["h"] = h
    if bad:
        out["status"] = PASSTHROUGH
        return out
    t = p32 - mn[None, :]                                          # float32
    q = t / h                                                      # a true fp32 division
    assert t.dtype == np.float32 and q.dtype == np.float32
    c = q.astype(np.int64)                                         # (int)q: q >= 0, truncation
    keys = ((c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]).astype(np.uint64)
    E = int(np.frexp(big)[1]) if big > 0 else 0
    s = np.ldexp(np.float64(1.0), 29 - E) if big > 0 else np.float64(1.0)
    Fx = np.rint(t.astype(np.float64) * s).astype(np.int64)        # exact product, ties to even
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.zeros((len(uniq), 3), np.int64)
    np.add.at(S, inv, Fx)
    nv = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    cen64 = mn.astype(np.float64)[None, :] + (S.astype(np.float64) / nv[:, None]) / s
    cen = cen64.astype(np.float32)                                 # the one rounding to fp32
    d = p32 - cen[inv]                                             # float32, every step rounded
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    pk = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(P, dtype=np.uint64)
    best = np.full(len(uniq), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    np.minimum.at(best, inv, pk)
    keep = np.zeros(P, np.int32)
    keep[first] = 1                                                # np.unique's first occurrence: the lowest member id
    centroids = np.zeros((P, 3), np.float32)
    centroids[first] = cen
    index = np.full(P, -1, np.int32)
    index[first] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
    centroids64 = np.zeros((P, 3), np.float64)
    centroids64[first] = cen64
    out.update(keep=keep, centroids=centroids, index=index, keys=keys, centroids64=centroids64)
    return out


# ---- compaction, batches ----------------------------------------------------------------------------------------------
def compact(clouds, sels, normals=None, use_selected=False):
    """The batch the device writes: points [new sum P, 3], index int32 [new sum P], normals or None, counts int32 [N],
    offsets int64 [N + 1].  sels: per-cloud dicts with keep and, with use_selected, centroids / index."""
    pts, idx, nrm, counts = [], [], [], []
    for i, (c, s) in enumerate(zip(clouds, sels)):
        p32 = np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3)
        if (s["status"] & 0xFF) in (EMPTY, TOO_LARGE, BAD_OFFSETS):
            counts.append(0)
            continue
        k = s["keep"] != 0
        src = s["index"][k] if use_selected else np.nonzero(k)[0].astype(np.int32)
        pts.append(s["centroids"][k] if use_selected else p32[k])
        idx.append(src.astype(np.int32))
        if normals is not None:
            nrm.append(np.asarray(normals[i], np.float32).reshape(-1, 3)[src])
        counts.append(int(k.sum()))
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum(counts)

    def cat(xs, shape, dt):
        return np.concatenate(xs).reshape(shape).astype(dt) if xs else np.zeros(0, dt).reshape(shape)
    return {"points": cat(pts, (-1, 3), np.float32), "index": cat(idx, (-1,), np.int32),
            "normals": None if normals is None else cat(nrm, (-1, 3), np.float32),
            "counts": np.array(counts, np.int32), "offsets": off}


def remove_outliers(clouds, k, std_ratio, normals=None, tables=None):
    """A batch through outlier selection and compaction: the compact() dict plus keep [sum P], mean_dist [sum P], stats
    [N, 3], status int32 [N]."""
    sels = [outlier_select_cloud(c, k, std_ratio, None if tables is None else tables[i]) for i, c in enumerate(clouds)]
    out = compact(clouds, sels, normals)
    out.update(keep=np.concatenate([s["keep"] for s in sels]), mean_dist=np.concatenate([s["mean_dist"] for s in sels]),
               stats=np.stack([s["stats"] for s in sels]), status=np.array([s["status"] for s in sels], np.int32))
    return out


def voxel_downsample(clouds, voxel, relative, normals=None):
    """A batch through voxel selection and compaction: the compact() dict plus keep, centroids, index_all (before the
    compaction, [sum P]) and status.  voxel: a number or one per cloud."""
    v = np.broadcast_to(np.asarray(voxel, np.float64).astype(np.float32), (len(clouds),))
    sels = [voxel_select_cloud(c, v[i], relative) for i, c in enumerate(clouds)]
    out = compact(clouds, sels, normals, use_selected=True)
    out.update(keep=np.concatenate([s["keep"] for s in sels]),
               centroids=np.concatenate([s["centroids"] for s in sels]).reshape(-1, 3),
               index_all=np.concatenate([s["index"] for s in sels]),
               status=np.array([s["status"] for s in sels], np.int32), sels=sels)
    return out


def split(batch, key="points"):
    """the per-cloud pieces of a compact() result"""
    off = batch["offsets"]
    return [batch[key][off[i]:off[i + 1]] for i in range(len(off) - 1)]
