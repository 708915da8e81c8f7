"""Anti-aliased renders, on the host: self-checks of the numpy restatement of the supersampling contract
(tests/render_ss_oracle.py), the argument codes of gv_render_prepare_ss / gv_render_draw_ss and the samples argument of
ViewRenderer.  No device."""
import ctypes as C

import numpy as np
import pytest
import torch                                       # noqa: F401  (before the library, as in the GPU test files)

from gvcnn_tf_amd import _lib, render as R

import render_oracle as O
import render_ss_oracle as SS
import test_gpu_render as G                         # its meshes (importing it touches no device)

F = np.float32


def descriptor(V, H, W, fov=0.0, two_sided=False, fit=0.9, elevation=30.0, azimuths=None, samples=1):
    """What ViewRenderer(...).descriptor() returns, without a device."""
    flags, k, D, a, b = R.projection(H, W, fov)
    return {"height": H, "width": W, "num_views": V, "flags": flags | (2 if two_sided else 0), "fit": float(F(fit)),
            "proj_scale": float(F(k)), "persp_dist": float(F(D)), "depth_a": float(F(a)), "depth_b": float(F(b)),
            "ambient": float(F(0.3)), "light": [float(F(x)) for x in R.DEFAULT_LIGHT],
            "color": [float(F(x)) for x in R.DEFAULT_COLOR], "background": [1.0, 1.0, 1.0],
            "cameras": R.camera_matrices(elevation, R.default_azimuths(V) if azimuths is None else azimuths),
            "samples": samples}


def snapped(mesh, d, v, rotation=None):
    verts, tris = mesh
    c, scale, st = O.normalise(verts, d["fit"])
    assert st == O.OK
    return O.project(O.world(verts, c, scale, rotation), d["cameras"][v], d) + (np.asarray(tris, np.int64),)


@pytest.mark.parametrize("fov,two_sided", [(0.0, False), (60.0, True)])
def test_one_sample_is_the_plain_oracle(fov, two_sided):
    batch = G.meshes()
    d = descriptor(2, 37, 29, fov=fov, two_sided=two_sided)
    rots = R.random_rotations(len(batch), "so3", seed=1)
    want, got = O.render(batch, d, rots), SS.render(batch, d, rots, samples=1)
    assert sorted(want) == sorted(got)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def direct_raster(X, Y, Z, tris, H, W, S):
    """every sample at its own position 256 i + step a + step / 2, unscaled coordinates, no bounding box."""
    step = 256 // S
    best = np.full((S * H, S * W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    PX = np.array([256 * i + step * a + step // 2 for i in range(W) for a in range(S)], np.int64)[None, :]
    PY = np.array([256 * j + step * b + step // 2 for j in range(H) for b in range(S)], np.int64)[:, None]
    for tid, (i0, i1, i2) in enumerate(tris):
        x0, y0, z0, x1, y1, z1, x2, y2, z2 = [int(q) for q in (X[i0], Y[i0], Z[i0], X[i1], Y[i1], Z[i1], X[i2], Y[i2],
                                                               Z[i2])]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        if area < 0:
            x1, y1, z1, x2, y2, z2 = x2, y2, z2, x1, y1, z1
            area = -area

        def edge(ax, ay, bx, by):
            return (bx - ax) * (PY - ay) - (by - ay) * (PX - ax)
        e0, e1, e2 = edge(x1, y1, x2, y2), edge(x2, y2, x0, y0), edge(x0, y0, x1, y1)
        cov = (((e0 > 0) | ((e0 == 0) & O.owns(x1, y1, x2, y2))) & ((e1 > 0) | ((e1 == 0) & O.owns(x2, y2, x0, y0))) &
               ((e2 > 0) | ((e2 == 0) & O.owns(x0, y0, x1, y1))))
        num = np.where(cov, e0 * z0 + e1 * z1 + e2 * z2, 0).astype(np.uint64)
        key = ((num // np.uint64(area)) << np.uint64(32)) | np.uint64(tid)
        np.copyto(best, np.minimum(best, key), where=cov)
    bg = best == np.uint64(0xFFFFFFFFFFFFFFFF)
    return (np.where(bg, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32),
            np.where(bg, np.uint64(0xFFFFFFFF), best >> np.uint64(32)).astype(np.uint32))


@pytest.mark.parametrize("fov", [0.0, 60.0])
def test_scaled_raster_equals_a_direct_sample_loop(fov):
    H, W = 37, 29
    d = descriptor(3, H, W, fov=fov)
    rot = R.random_rotations(1, "so3", seed=2)[0]
    hits = 0
    for mesh, v, r in ((R.icosphere(2), 0, None), (SS.thin_strip(), 0, None), (G.duplicates(), 1, None),
                       (G.giant_tiny(), 2, rot)):
        X, Y, Z, tris = snapped(mesh, d, v, r)
        for S in (1, 2, 4):
            fa, da = SS.raster(X, Y, Z, tris, H, W, S)
            fb, db = direct_raster(X, Y, Z, tris, H, W, S)
            assert fa.shape == (S * H, S * W) and fa.tobytes() == fb.tobytes() and da.tobytes() == db.tobytes()
            hits += int((fa >= 0).sum())
    assert hits > 1000


def test_resolve_u8_rounds_half_up():
    for S in (1, 2, 4):
        n = S * S
        for total in (0, n // 2 - 1, n // 2, n // 2 + 1, n, 3 * n + n // 2 - 1, 3 * n + n // 2, 255 * n - n // 2 - 1,
                      255 * n - n // 2, 255 * n):
            if total < 0:
                continue
            s = np.zeros((1, 1, n, 3), np.uint8)                        # hand-made samples adding up to `total`
            left = total
            for i in range(n):
                s[0, 0, i, :] = min(left, 255)
                left -= min(left, 255)
            assert left == 0
            want = int(np.floor(total / n + 0.5))                       # the mean, halves rounded up
            assert SS.resolve_u8(s, S).tolist() == [[[want] * 3]], (S, total)
    s = np.zeros((1, 1, 4, 3), np.uint8)
    s[0, 0, :, 0], s[0, 0, :, 1], s[0, 0, :, 2] = [255, 255, 255, 254], [1, 0, 0, 0], [1, 1, 0, 0]
    assert SS.resolve_u8(s, 2).tolist() == [[[255, 0, 1]]]             # 1019 / 4 -> 255, 1 / 4 -> 0, 2 / 4 -> 1
    assert SS.resolve_u8(s.astype(np.uint8)[:, :, :1], 1).tolist() == [[[255, 1, 1]]]


def test_resolve_f32_adds_in_sample_order():
    big, one = F(2.0 ** 24), F(1.0)
    a = np.array([big, one, one, one], np.float32).reshape(1, 1, 4, 1)   # (big + 1) + 1 + 1 = big: each add rounds
    b = np.array([one, one, one, big], np.float32).reshape(1, 1, 4, 1)   # 1 + 1 + 1 + big = big + 4 (3 rounds to even)
    ra, rb = SS.resolve_f32(a, 2), SS.resolve_f32(b, 2)
    assert ra.dtype == np.float32 and ra.shape == (1, 1, 1)
    assert float(ra[0, 0, 0]) == float(F(F(big * F(0.25)) + F(-0.5)))
    assert float(rb[0, 0, 0]) == float(F(F(F(big + F(4.0)) * F(0.25)) + F(-0.5)))
    assert float(ra[0, 0, 0]) != float(rb[0, 0, 0])
    c = np.array([0.1, 0.7, 0.3, 0.9], np.float32).reshape(1, 1, 4, 1)
    want = F(F(F(F(F(0.1) + F(0.7)) + F(0.3)) + F(0.9)) * F(0.25)) + F(-0.5)
    assert SS.resolve_f32(c, 2).tobytes() == np.array([want], np.float32).tobytes()
    assert SS.resolve_f32(c[:, :, :1], 1).tobytes() == np.array([F(0.1) + F(-0.5)], np.float32).tobytes()
    # the row-major order of a pixel's samples: b (rows) outer, a (columns) inner
    grid = np.arange(2 * 4 * 4 * 1, dtype=np.float32).reshape(2, 4, 4, 1)           # [image, S*H, S*W, C], S = 2
    s = SS.split_samples(grid, 2)
    assert s.shape == (2, 2, 2, 4, 1)
    assert s[0, 0, 1, :, 0].tolist() == [2.0, 3.0, 6.0, 7.0] and s[1, 1, 0, :, 0].tolist() == [24.0, 25.0, 28.0, 29.0]


def test_thin_strip_survives_supersampling():
    H, W = 37, 29
    d = descriptor(3, H, W)
    X, Y, Z, tris = snapped(SS.thin_strip(), d, 0)
    f1, _ = SS.raster(X, Y, Z, tris, H, W, 1)
    f4, _ = SS.raster(X, Y, Z, tris, H, W, 4)
    rows1 = int((f1 >= 0).any(axis=1).sum())
    rows4 = int((f4 >= 0).reshape(H, 4, 4 * W).any(axis=(1, 2)).sum())
    assert rows4 > rows1
    out1, out4 = SS.render([SS.thin_strip()], d, samples=1), SS.render([SS.thin_strip()], d, samples=4)
    assert (out4["u8"][0, 0] != 255).any(axis=(1, 2)).sum() > (out1["u8"][0, 0] != 255).any(axis=(1, 2)).sum()


def test_sample_box_binning_matches_the_plain_one():
    batch = [R.icosphere(2), G.soup(), SS.thin_strip()]
    d = descriptor(2, 37, 29, fov=60.0)
    assert SS.tile_counts(batch, d, samples=1).tobytes() == O.tile_counts(batch, d).tobytes()
    c1, c4 = SS.tile_counts(batch, d, samples=1), SS.tile_counts(batch, d, samples=4)
    assert (c4 >= c1).all() and c4.sum() > c1.sum()                     # triangles that cover a sample but no centre


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def desc(**kw):
    d = _lib.RenderDesc()
    d.height, d.width, d.num_views, d.flags = 64, 48, 4, 0
    d.fit, d.proj_scale, d.ambient = 0.9, 24.0, 0.3
    for i in range(3):
        d.light[i], d.color[i], d.background[i] = (-2 / 3, -2 / 3, 1 / 3)[i], 0.5, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_ss_abi_argument_codes():
    """Every rejection happens before any HIP call (this runs without a device)."""
    lib = _lib.load()
    P = 4096                                             # a 16-byte aligned stand-in address: never dereferenced
    WS = lib.gv_render_workspace_bytes(2, 4, 64, 48, 10)
    assert WS > 0

    def prep(d, samples=2, **kw):
        a = dict(verts=P, vo=P, tris=P, to=P, n=2, nv=6, nt=10, mt=5, cams=P, rots=None, ws=P, wsb=WS, total=P,
                 status=P)
        a.update(kw)
        return lib.gv_render_prepare_ss(a["verts"], a["vo"], a["tris"], a["to"], a["n"], a["nv"], a["nt"], a["mt"],
                                        C.byref(d) if d is not None else None, a["cams"], a["rots"], a["ws"], a["wsb"],
                                        a["total"], a["status"], samples, None)

    def draw(d, samples=2, **kw):
        a = dict(verts=P, vo=P, tris=P, to=P, n=2, nv=6, nt=10, mt=5, cams=P, rots=None, ws=P, wsb=WS, bins=P,
                 binsb=256, total=10, output=_lib.GV_RENDER_OUT_U8, out=P, face=None, depth=None)
        a.update(kw)
        return lib.gv_render_draw_ss(a["verts"], a["vo"], a["tris"], a["to"], a["n"], a["nv"], a["nt"], a["mt"],
                                     C.byref(d) if d is not None else None, a["cams"], a["rots"], a["ws"], a["wsb"],
                                     a["bins"], a["binsb"], a["total"], a["output"], a["out"], a["face"], a["depth"],
                                     samples, None)

    for fn in (prep, draw):
        for bad in (0, -1, -4, 3, 5, 6, 7, 12, 255, -(2 ** 31)):
            assert fn(desc(), samples=bad) == _lib.GV_E_BADARG, bad
        for big in (8, 16, 256, 2 ** 30):
            assert fn(desc(), samples=big) == _lib.GV_E_UNSUPPORTED, big
        for ok in (1, 2, 4):                                               # the shared rejections, whatever S
            assert fn(None, samples=ok) == -1
            for name in ("verts", "vo", "tris", "to", "cams", "ws"):
                assert fn(desc(), samples=ok, **{name: None}) == -1, name
            assert fn(desc(), samples=ok, n=0) == -1
            assert fn(desc(), samples=ok, mt=-1) == -1
            assert fn(desc(), samples=ok, wsb=WS - 1) == -1
            for bad in (dict(height=0), dict(flags=4), dict(fit=1.5), dict(ambient=-0.1), dict(proj_scale=0.0),
                        dict(flags=_lib.GV_RENDER_PERSPECTIVE, persp_dist=1.0)):
                assert fn(desc(**bad), samples=ok) == -1, bad
            assert fn(desc(height=513), samples=ok) == -2
            assert fn(desc(width=513), samples=ok) == -2
            assert fn(desc(num_views=65), samples=ok) == -2
            assert fn(desc(), samples=ok, mt=(1 << 24) + 1) == -2
            assert fn(desc(), samples=ok, ws=P + 8) == -3
    for ok in (1, 2, 4):
        assert prep(desc(), samples=ok, total=None) == -1
        assert prep(desc(), samples=ok, status=None) == -1
        assert draw(desc(), samples=ok, bins=None) == -1
        assert draw(desc(), samples=ok, out=None) == -1
        assert draw(desc(), samples=ok, output=3) == -1
        assert draw(desc(), samples=ok, total=65, binsb=256) == -1
        assert draw(desc(), samples=ok, bins=P + 4) == -3
        assert draw(desc(), samples=ok, output=_lib.GV_RENDER_OUT_F32, out=P + 2) == -3
        assert draw(desc(), samples=ok, face=P + 2) == -3
    assert lib.gv_abi_version() == 1


def test_samples_argument_is_checked_first(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before samples was checked")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in (0, 3, 8, -2, 1.5, None, "2"):
        with pytest.raises(ValueError, match="samples"):
            R.ViewRenderer(2, 16, 16, samples=bad)
