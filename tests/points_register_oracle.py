"""numpy restatement of the registration contract (include/gvcnn_hip.h, "points in", registration), step by step in fp64
and fp32: the move formula, a brute-force table of nearest keys, the tree sum as pairs of a reshaped array, the 4x4 cyclic
Jacobi in scalar float64, Horn's quaternion and the rounds' stopping rules.  No grid: this is the answer the device's grid,
cell order and schedule must not change."""
import numpy as np

F = np.float32
D = np.float64
OK, EMPTY = 0, 1                                                   # GV_RENDER_*
CONVERGED, FEW_PAIRS, NONFINITE = 0x800, 0x1000, 0x2000            # GV_POINTS_ICP_*
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
CHUNK = 512


def move(T, p32):
    """q_c = ((R_c0 x + R_c1 y) + R_c2 z) + t_c in fp64, rounded once to fp32.  T: [3 or 4, 4] float64."""
    p = np.ascontiguousarray(p32, dtype=F).reshape(-1, 3).astype(D)
    T = np.asarray(T, D)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.stack([((T[c, 0] * p[:, 0] + T[c, 1] * p[:, 1]) + T[c, 2] * p[:, 2]) + T[c, 3] for c in range(3)], axis=1)
        return q.astype(F)


def rotate(T, g32):
    """normals: ((R_c0 x + R_c1 y) + R_c2 z) in fp64, rounded once."""
    g = np.ascontiguousarray(g32, dtype=F).reshape(-1, 3).astype(D)
    T = np.asarray(T, D)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([(T[c, 0] * g[:, 0] + T[c, 1] * g[:, 1]) + T[c, 2] * g[:, 2] for c in range(3)], axis=1).astype(F)


def nearest_keys(q32, y32):
    """uint64 [P]: per moved source point the smallest key (bits(d2) << 32 | j) over every target point j."""
    q = np.ascontiguousarray(q32, dtype=F).reshape(-1, 3)
    y = np.ascontiguousarray(y32, dtype=F).reshape(-1, 3)
    ids = np.arange(len(y), dtype=np.uint64)
    out = np.zeros(len(q), np.uint64)
    for a in range(0, len(q), CHUNK):
        c = q[a:a + CHUNK]
        with np.errstate(over="ignore"):
            dx = y[None, :, 0] - c[:, None, 0]                     # float32 throughout: one rounding per step
            dy = y[None, :, 1] - c[:, None, 1]
            dz = y[None, :, 2] - c[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        out[a:a + CHUNK] = ((d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]).min(axis=1)
    return out


def tree_sum(a):
    """T(a) per column of a [P] or [P, C]: zeros up to the next power of two, then adjacent pairs level by level."""
    a = np.asarray(a, D)
    a = a.reshape(len(a), -1)
    n = 1
    while n < len(a):
        n *= 2
    b = np.zeros((n, a.shape[1]), D)
    b[:len(a)] = a
    with np.errstate(over="ignore", invalid="ignore"):
        while len(b) > 1:
            pairs = b.reshape(len(b) // 2, 2, -1)
            b = pairs[:, 0] + pairs[:, 1]
    return b[0]


def horn_matrix(H):
    H = np.asarray(H, D)
    A = np.zeros((4, 4), D)
    A[0, 0] = (H[0, 0] + H[1, 1]) + H[2, 2]
    A[1, 1] = (H[0, 0] - H[1, 1]) - H[2, 2]
    A[2, 2] = (H[1, 1] - H[0, 0]) - H[2, 2]
    A[3, 3] = (H[2, 2] - H[0, 0]) - H[1, 1]
    A[0, 1] = A[1, 0] = H[1, 2] - H[2, 1]
    A[0, 2] = A[2, 0] = H[2, 0] - H[0, 2]
    A[0, 3] = A[3, 0] = H[0, 1] - H[1, 0]
    A[1, 2] = A[2, 1] = H[0, 1] + H[1, 0]
    A[1, 3] = A[3, 1] = H[2, 0] + H[0, 2]
    A[2, 3] = A[3, 2] = H[1, 2] + H[2, 1]
    return A


def jacobi4(A):
    """(diagonal [4], V [4, 4]) after SWEEPS cyclic sweeps over PAIRS, scalar float64, the normals' rotation formulas."""
    A = np.array(A, D)
    V = np.eye(4, dtype=D)
    one, two = D(1.0), D(2.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (two * apq)
                t = (D(-1.0) if theta < 0.0 else one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                A[p, p] = A[p, p] - h
                A[q, q] = A[q, q] + h
                A[p, q] = A[q, p] = 0.0
                for r in range(4):
                    if r in (p, q):
                        continue
                    x, y = A[r, p], A[r, q]
                    A[r, p] = A[p, r] = c * x - s * y
                    A[r, q] = A[q, r] = s * x + c * y
                for i in range(4):
                    x, y = V[i, p], V[i, q]
                    V[i, p] = c * x - s * y
                    V[i, q] = s * x + c * y
    return np.diag(A).copy(), V


def quaternion(H):
    """the unit quaternion (w, x, y, z) of Horn's closed form for H = sum (p - cp)(y - cy)^T"""
    lam, V = jacobi4(horn_matrix(H))
    col = 0
    for c in range(1, 4):
        if lam[c] > lam[col]:
            col = c
    e = V[:, col].copy()
    nz = [v for v in e if v != 0.0]
    if nz and nz[0] < 0.0:
        e = -e
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nn = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]
        return e / np.sqrt(nn)


def rotation(quat):
    w, x, y, z = [D(v) for v in quat]
    two = D(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([[((w * w + x * x) - y * y) - z * z, two * (x * y - w * z), two * (x * z + w * y)],
                         [two * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, two * (y * z - w * x)],
                         [two * (x * z - w * y), two * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]], D)


def horn(H):
    """R float64 [3, 3] of Horn's closed form"""
    return rotation(quaternion(H))


def solve(H, cp, cy):
    """T float64 [3, 4]: R of Horn and t = cy - R cp in the contract's order"""
    R = horn(H)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.array([cy[c] - ((R[c, 0] * cp[0] + R[c, 1] * cp[1]) + R[c, 2] * cp[2]) for c in range(3)], D)
    return np.concatenate([R, t[:, None]], axis=1)


def max_d2_of(max_distance):
    md = F(np.inf if max_distance is None else max_distance)
    with np.errstate(over="ignore"):
        return md * md


def register_pair(source, target, init=None, iterations=30, max_distance=None, tolerance=0.0, normals=None):
    """One pair: dict transform float64 [4, 4], rmse float64, inliers / used int, correspondence int32 [Ps], moved float32
    [Ps, 3], moved_normals or None, status int; and for the tests history: the rmse of every round run."""
    p32 = np.ascontiguousarray(source, dtype=F).reshape(-1, 3)
    y32 = np.ascontiguousarray(target, dtype=F).reshape(-1, 3)
    assert np.isfinite(p32).all() and np.isfinite(y32).all()
    T = np.eye(4, dtype=D)[:3] if init is None else np.array(init, D).reshape(4, 4)[:3].copy()
    P = len(p32)
    out = {"rmse": D(0.0), "inliers": 0, "used": 0, "correspondence": np.full(P, -1, np.int32), "history": []}
    byte = EMPTY if P == 0 or len(y32) == 0 else OK
    flags = 0
    max_d2 = max_d2_of(max_distance)
    tol = D(tolerance)
    prev = None
    pd = p32.astype(D)
    for k in range(1, iterations + 1):
        if byte != OK:
            break
        out["used"] = k
        q = move(T, p32)
        if not np.isfinite(q).all():
            flags |= NONFINITE
            out.update(inliers=0, rmse=D(0.0), correspondence=np.full(P, -1, np.int32))
            break
        keys = nearest_keys(q, y32)
        match = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        inl = d2 <= max_d2
        yd = y32[match].astype(D)
        zero = np.zeros(P, D)
        first = np.stack([np.where(inl, 1.0, zero)] + [np.where(inl, pd[:, c], zero) for c in range(3)] +
                         [np.where(inl, yd[:, c], zero) for c in range(3)] + [np.where(inl, d2.astype(D), zero)], axis=1)
        tot = tree_sum(first)
        cnt = tot[0]
        out["inliers"] = int(cnt)
        out["correspondence"] = np.where(inl, match, -1).astype(np.int32)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if cnt < 3.0:
                flags |= FEW_PAIRS
                out["rmse"] = np.sqrt(tot[7] / cnt) if cnt > 0.0 else D(0.0)
                out["history"].append(out["rmse"])
                break
            rmse = np.sqrt(tot[7] / cnt)
            out["rmse"] = rmse
            out["history"].append(rmse)
            if k > 1 and np.abs(prev - rmse) <= tol:
                flags |= CONVERGED
                break
            prev = rmse
            cp, cy = tot[1:4] / cnt, tot[4:7] / cnt
            ep, ey = pd - cp[None, :], yd - cy[None, :]
            second = np.stack([np.where(inl, ep[:, a] * ey[:, b], zero) for a in range(3) for b in range(3)], axis=1)
        H = tree_sum(second).reshape(3, 3)
        T = solve(H, cp, cy)
    full = np.eye(4, dtype=D)
    full[:3] = T
    out.update(transform=full, moved=move(T, p32), status=byte | flags,
               moved_normals=None if normals is None else rotate(T, normals))
    return out


def register(sources, targets, init=None, iterations=30, max_distance=None, tolerance=0.0, normals=None):
    """A batch: the arrays the device writes, concatenated as it lays them out, plus pairs (the per-pair dicts)."""
    n = len(sources)
    assert len(targets) == n
    pairs = [register_pair(sources[i], targets[i], None if init is None else np.asarray(init, D).reshape(-1, 4, 4)[i],
                           iterations, max_distance, tolerance, None if normals is None else normals[i]) for i in range(n)]

    def cat(key, shape, dt):
        xs = [np.asarray(p[key], dt).reshape(shape) for p in pairs]
        return np.concatenate(xs).reshape(shape).astype(dt)
    return {"transforms": np.stack([p["transform"] for p in pairs]).astype(D),
            "rmse": np.array([p["rmse"] for p in pairs], D), "inliers": np.array([p["inliers"] for p in pairs], np.int32),
            "used": np.array([p["used"] for p in pairs], np.int32), "correspondence": cat("correspondence", (-1,), np.int32),
            "moved": cat("moved", (-1, 3), F),
            "moved_normals": None if normals is None else cat("moved_normals", (-1, 3), F),
            "status": np.array([p["status"] for p in pairs], np.int32), "pairs": pairs}


# ---- helpers of the tests -----------------------------------------------------------------------------------------------
def axis_angle(axis, degrees):
    """float64 rotation matrix (Rodrigues)"""
    a = np.asarray(axis, D)
    a = a / np.linalg.norm(a)
    th = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], D)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rigid(R, t):
    T = np.eye(4, dtype=D)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def box_surface(n, edges=(1.0, 0.6, 0.3), seed=0):
    """n points on the surface of an axis-aligned box centred on the origin, float32: faces drawn by area"""
    rng = np.random.RandomState(seed)
    e = np.asarray(edges, D)
    area = np.array([e[1] * e[2], e[0] * e[2], e[0] * e[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    p = rng.uniform(-0.5, 0.5, size=(n, 3)) * e[None, :]
    p[np.arange(n), axis] = np.where(rng.rand(n) < 0.5, -0.5, 0.5) * e[axis]
    return p.astype(F)
