"""numpy restatement of the normal-estimation contract (include/gvcnn_hip.h, "points in", normal estimation): brute-force
neighbours from fp32 squared distances with every step rounded on its own and uint64 keys, the fp64 covariance in rank
order, the same cyclic Jacobi, the same degenerate and sign rules.  No grid: this is the answer the device's search grid
must not change."""
import numpy as np

F = np.float32
OK, EMPTY, NONFINITE = 0, 1, 3                                     # GV_RENDER_*
DEGENERATE = 0x100                                                 # GV_POINTS_DEGENERATE_NORMAL
MIN_K, MAX_K = 3, 32
SWEEPS = 6
CHUNK = 512                                                        # query rows per block: 512 x 5 000 keys = 20 MB
ORIENTS = ("none", "outward", "viewpoint")


def neighbours(points, k):
    """ids int32 [P, k] of the k_eff = min(k, P) smallest keys (bits(d2) << 32 | j) per point in ascending order, -1
    beyond k_eff."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(p)
    keff = min(k, P)
    out = np.full((P, k), -1, np.int32)
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
        if keff < P:
            keys = np.partition(keys, keff - 1, axis=1)[:, :keff]
        keys = np.sort(keys, axis=1)
        out[a:a + CHUNK, :keff] = (keys & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return out


def covariance(points, nb, keff):
    """(C00, C01, C02, C11, C12, C22) float64 [P] each, of the neighbourhoods nb[:, :keff] in rank order."""
    p = np.asarray(points, np.float32).astype(np.float64)
    P = len(p)
    d = [p[nb[:, r]] - p for r in range(keff)]                     # d_r = (double)p_r - (double)p_i
    s = np.zeros((P, 3))
    for r in range(keff):
        s = s + d[r]
    m = s / np.float64(keff)
    C = [np.zeros(P) for _ in range(6)]
    for r in range(keff):
        e = d[r] - m
        for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[n] = C[n] + e[:, i] * e[:, j]
    return C


def jacobi(C, sweeps=SWEEPS):
    """Cyclic Jacobi of symmetric 3x3 matrices given as the six arrays of covariance(): (diag [P, 3], V [P, 3, 3]) with
    V's columns the eigenvectors, unsorted.  Pairs (0,1), (0,2), (1,2); a pair whose entry is exactly 0 is skipped."""
    P = len(C[0])
    A = {(0, 0): C[0].copy(), (0, 1): C[1].copy(), (0, 2): C[2].copy(), (1, 1): C[3].copy(), (1, 2): C[4].copy(),
         (2, 2): C[5].copy()}
    V = np.zeros((P, 3, 3))
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0

    def key(i, j):
        return (i, j) if i <= j else (j, i)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[(p, q)]
                on = apq != 0.0
                safe = np.where(on, apq, 1.0)
                theta = (A[(q, q)] - A[(p, p)]) / (2.0 * safe)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * safe
                arp, arq = A[key(r, p)], A[key(r, q)]
                new = {(p, p): A[(p, p)] - h, (q, q): A[(q, q)] + h, (p, q): np.zeros(P),
                       key(r, p): c * arp - s * arq, key(r, q): s * arp + c * arq}
                for kk, val in new.items():
                    A[kk] = np.where(on, val, A[kk])
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([A[(0, 0)], A[(1, 1)], A[(2, 2)]], axis=1), V


def flip_none(n):
    """the "none" rule: negate when the component of largest magnitude (the first of x, y, z on a tie) is negative"""
    lead = np.argmax(np.abs(n), axis=1)                            # argmax takes the first maximum
    return n[np.arange(len(n)), lead] < 0.0


def estimate_cloud(points, k, orient="outward", viewpoint=None, nb=None):
    """One cloud: dict normals float32 [P, 3], neighbours int32 [P, k], variation float32 [P], status int.  nb: the
    cloud's neighbours(points, k') for some k' >= k, when the caller has them (the k smallest keys are a prefix)."""
    assert MIN_K <= k <= MAX_K and orient in ORIENTS and (viewpoint is not None) == (orient == "viewpoint")
    p32 = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(p32)
    out = {"normals": np.zeros((P, 3), np.float32), "neighbours": np.full((P, k), -1, np.int32),
           "variation": np.zeros(P, np.float32), "status": OK}
    if P == 0:
        out["status"] = EMPTY
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        ext = p32.max(axis=0) - p32.min(axis=0)
    if not np.isfinite(p32).all() or not np.isfinite(ext).all():
        out["status"] = NONFINITE
        return out
    keff = min(k, P)
    if nb is None:
        nb = neighbours(p32, k)
    out["neighbours"][:, :keff] = nb[:, :keff]
    if keff < 3:
        out["status"] |= DEGENERATE
        return out
    diag, V = jacobi(covariance(p32, nb, keff))
    # l0 <= l1 <= l2, ties by column index: a stable sort of the diagonal
    order = np.argsort(diag, axis=1, kind="stable")
    rows = np.arange(P)
    l0, l1, l2 = (diag[rows, order[:, i]] for i in range(3))
    n = V[rows, :, order[:, 0]]                                    # column c0 of V, [P, 3]
    bad = (l2 == 0.0) | (l1 <= 1e-12 * l2)
    p = p32.astype(np.float64)
    flip = flip_none(n)
    if orient != "none":
        if orient == "outward":
            w = p - 0.5 * (p32.min(axis=0).astype(np.float64) + p32.max(axis=0).astype(np.float64))
        else:
            w = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - p
        d = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
        flip = np.where(d == 0.0, flip, d < 0.0)
    n = np.where(flip[:, None], -n, n)
    with np.errstate(all="ignore"):
        var = l0 / ((l0 + l1) + l2)
    out["normals"] = np.where(bad[:, None], 0.0, n).astype(np.float32)
    out["variation"] = np.where(bad, 0.0, var).astype(np.float32)
    if bad.any():
        out["status"] |= DEGENERATE
    return out


def estimate(clouds, k, orient="outward", viewpoint=None, nbs=None):
    """A batch: the clouds' results concatenated as the device lays them out (normals [sum P, 3], neighbours [sum P, k],
    variation [sum P], status int32 [N]).  nbs: per-cloud neighbour tables as estimate_cloud's nb."""
    res = [estimate_cloud(c, k, orient, viewpoint, None if nbs is None else nbs[i]) for i, c in enumerate(clouds)]
    return {"normals": np.concatenate([r["normals"] for r in res]).reshape(-1, 3),
            "neighbours": np.concatenate([r["neighbours"] for r in res]).reshape(-1, k),
            "variation": np.concatenate([r["variation"] for r in res]),
            "status": np.array([r["status"] for r in res], np.int32)}
