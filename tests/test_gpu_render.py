"""Meshes in, on the device: the rasteriser against the numpy restatement of its contract (tests/render_oracle.py), bit
for bit; batch invariance; status codes; the PNG / TFRecord round trip; the engine entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gvcnn_tf_amd as gv                          # noqa: E402
from gvcnn_tf_amd import records, render as R      # noqa: E402

import render_oracle as O                          # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(t):
    torch.cuda.synchronize()
    if t.dtype in (torch.bfloat16, torch.float16):                     # compared bit for bit: keep the raw bits
        t = t.view(torch.int16)
    return t.cpu().numpy()


# ---- meshes --------------------------------------------------------------------------------------------------------
def cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * 0.7 + [0.3, -0.2, 0.1]
    t = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return v, np.array(t, np.int32)


def tetra():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * 3.0
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


def soup(n=48, seed=5):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, size=(n, 1, 3))
    v = (c + rng.uniform(-0.6, 0.6, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def duplicates():
    """coplanar duplicate triangles: the lower id must win every shared pixel."""
    v = np.array([[0, -1, -1], [0, 1, -1], [0, 0, 1], [0, 1, 1], [0, -1, 0.5]], np.float32)
    return v, np.array([(0, 1, 2), (0, 1, 2), (2, 1, 0), (0, 3, 4), (1, 3, 4)], np.int32)


def quad():
    """two triangles spanning most of the screen (facing +x)."""
    v = np.array([[0, -1, -1], [0, 1, -1], [0, 1, 1], [0, -1, 1]], np.float32)
    return v, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def giant_tiny(n=150, seed=7):
    rng = np.random.RandomState(seed)
    qv, qt = quad()
    c = rng.uniform(-0.9, 0.9, size=(n, 1, 3))
    c[:, 0, 0] = rng.uniform(-0.5, 0.5, size=n)                        # in front of the quad or behind it
    small = (c + rng.uniform(-0.02, 0.02, size=(n, 3, 3))).reshape(-1, 3)
    v = np.concatenate([qv, small]).astype(np.float32)
    t = np.concatenate([qt, 4 + np.arange(3 * n).reshape(n, 3)]).astype(np.int32)
    return v, t


def dense(n=1500, seed=11):
    """many small triangles packed round the centre (an anchor triangle sets the radius): long lists in few tiles."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-0.12, 0.12, size=(n, 1, 3))
    v = (c + rng.uniform(-0.03, 0.03, size=(n, 3, 3))).reshape(-1, 3)
    anchor = np.array([[0, 1, 0], [0, 0.95, 0.05], [0.05, 0.95, 0]])
    return np.concatenate([v, anchor]).astype(np.float32), np.arange(3 * n + 3, dtype=np.int32).reshape(n + 1, 3)


def meshes():
    return [cube(), tetra(), R.icosphere(2), soup(), duplicates(), giant_tiny()]


def stride_all_chunks(batch):
    """make the binning grid one workgroup per image, so the grid-stride loop walks every chunk of triangles (the
    grid size is a hint of the C ABI: the results must not depend on it)."""
    group = batch.group
    batch.group = lambda a, b: group(a, b)[:7] + (1,)
    return batch


def check_equal(r, batch, rotations=None, quantize_too=True):
    want = O.render(batch, r.descriptor(), rotations)
    out, face, depth = r.render(batch, rotations=rotations, return_buffers=True)
    f, d = host(face), host(depth).view(np.uint32)
    np.testing.assert_array_equal(f, want["face_id"])
    np.testing.assert_array_equal(d, want["depth"])
    assert host(out).tobytes() == want["f32q"].tobytes()
    assert host(r.render_uint8(batch, rotations=rotations)).tobytes() == want["u8"].tobytes()
    if quantize_too:
        assert host(r.render(batch, rotations=rotations, quantize=False)).tobytes() == want["f32"].tobytes()
    np.testing.assert_array_equal(r.status, want["status"])
    return want


CASES = [  # (V, H, W, kwargs, rotations)
    (1, 64, 64, {}, None),
    (3, 48, 80, {"fov": 60.0, "two_sided": True}, "so3"),
    (12, 64, 64, {}, "z"),
    (4, 80, 48, {"fov": 45.0, "elevation": -20.0}, None),
    (2, 40, 40, {"two_sided": True, "fit": 1.0, "ambient": 0.5}, "so3"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_equals_oracle(case):
    V, H, W, kw, rot = CASES[case]
    batch = meshes()
    r = R.ViewRenderer(V, H, W, device=DEV, **kw)
    rots = None if rot is None else R.random_rotations(len(batch), rot, seed=case)
    want = check_equal(r, batch, rots)
    assert (want["status"] == 0).all()
    assert (want["face_id"] >= 0).sum() > 0.05 * want["face_id"].size          # the pictures are not empty


@pytest.mark.parametrize("fov", [0.0, 60.0])
def test_large_meshes_equal_oracle(fov):
    """More than one binning workgroup per image (1024 triangles each), tile lists longer than one LDS pass (256),
    and the grid-stride loop of a one-workgroup grid."""
    batch = [R.icosphere(4), dense()]
    r = R.ViewRenderer(2, 40, 48, fov=fov, device=DEV)
    rots = R.random_rotations(2, "so3", seed=9)
    counts = O.tile_counts(batch, r.descriptor(), rots)
    assert min(len(t) for _, t in batch) > 1024 and counts[0].max() > 2 * 256 and counts[1].max() > 256
    want = check_equal(r, batch, rots, quantize_too=False)
    assert (want["face_id"] >= 0).sum() > 0.1 * want["face_id"].size
    strided = R.MeshBatch(batch, DEV)
    stride_all_chunks(strided)
    f, d = r.render(strided, rotations=rots, return_buffers=True)[1:]
    np.testing.assert_array_equal(host(f), want["face_id"])
    np.testing.assert_array_equal(host(d).view(np.uint32), want["depth"])


def test_rotations_must_be_rotations():
    r = R.ViewRenderer(1, 16, 16, device=DEV)
    for bad in (np.eye(3, dtype=np.float32)[None] * 20, np.diag([1.0, 1.0, -1.0]).astype(np.float32)[None],
                np.full((1, 3, 3), np.nan, np.float32), np.eye(3, dtype=np.float32)[None].repeat(2, 0)):
        with pytest.raises(ValueError):
            r.render([cube()], rotations=bad)


def test_device_spellings():
    r = R.ViewRenderer(2, 16, 16, device="cuda")
    out = torch.empty((1, 2, 16, 16, 3), dtype=torch.float32, device=DEV)
    assert r.render([cube()], out=out) is out
    assert host(r.render(R.MeshBatch([cube()], "cuda"))).tobytes() == host(out).tobytes()


def test_duplicates_lower_id_wins():
    r = R.ViewRenderer(2, 32, 32, azimuths=[0.0, 180.0], elevation=0.0, device=DEV)
    want = check_equal(r, [duplicates()])
    f = want["face_id"]
    assert not np.isin(f, [1, 2]).any() and (f == 0).any()


@pytest.mark.parametrize("fov", [0.0, 90.0])
def test_full_screen_quad_299(fov):
    r = R.ViewRenderer(1, 299, 299, azimuths=[0.0], elevation=0.0, fit=1.0, fov=fov, device=DEV)
    want = check_equal(r, [quad(), giant_tiny()], quantize_too=False)
    assert (want["face_id"][0] >= 0).sum() > 0.2 * 299 * 299


def test_batch_invariance_and_determinism():
    A, B, C = R.icosphere(4), soup(), dense()                  # A: 5 binning workgroups, lists past one LDS pass
    r = R.ViewRenderer(5, 56, 72, device=DEV)
    rots = R.random_rotations(3, "so3", seed=3)
    assert O.tile_counts([A, C], r.descriptor(), rots[[0, 2]]).max() > 256
    all3 = [host(t) for t in r.render([A, B, C], rotations=rots, return_buffers=True)]
    for i, m in enumerate((A, B, C)):
        one = [host(t) for t in r.render([m], rotations=rots[i:i + 1], return_buffers=True)]
        for x, y in zip(all3, one):
            assert x[i:i + 1].tobytes() == y.tobytes()
    tiny = R.ViewRenderer(5, 56, 72, device=DEV, max_workspace_bytes=1)           # forced to one mesh per group
    split = [host(t) for t in tiny.render([A, B, C], rotations=rots, return_buffers=True)]
    for x, y in zip(all3, split):
        assert x.tobytes() == y.tobytes()
    rev = [host(t) for t in r.render([C, B, A], rotations=rots[::-1].copy(), return_buffers=True)]
    for x, y in zip(all3, rev):
        assert x.tobytes() == y[::-1].tobytes()
    batch = R.MeshBatch([A, B, C], DEV)
    again = [host(r.render(batch, rotations=rots)) for _ in range(3)]
    again.append(host(r.render(stride_all_chunks(R.MeshBatch([A, B, C], DEV)), rotations=rots)))
    assert again[0].tobytes() == again[1].tobytes() == again[2].tobytes() == again[3].tobytes() == all3[0].tobytes()


def test_empty_and_degenerate_meshes():
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    point = (np.ones((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    flat = (np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    no_tris = (np.ones((4, 3), np.float32), np.zeros((0, 3), np.int32))
    r = R.ViewRenderer(2, 32, 32, device=DEV)
    out, face, depth = r.render([empty, cube(), point, flat, no_tris], return_buffers=True)
    st = r.status
    assert st.tolist() == [gv._lib.GV_RENDER_EMPTY, 0, gv._lib.GV_RENDER_ZERO_RADIUS, 0, gv._lib.GV_RENDER_EMPTY]
    f, d, o = host(face), host(depth).view(np.uint32), host(out)
    bg = np.float32(255 * np.float64(np.float32(1 / 255)) - 0.5)                 # fma(255, 1/255, -0.5), one rounding
    for i in (0, 2, 4):
        assert (f[i] == -1).all() and (d[i] == 0xFFFFFFFF).all() and (o[i] == bg).all()
    assert (f[1] >= 0).any()


def test_png_record_round_trip(tmp_path):
    N, V, H, W = 3, 4, 40, 48
    batch = [cube(), R.icosphere(1), tetra()]
    r = R.ViewRenderer(V, H, W, device=DEV)
    u8 = host(r.render_uint8(batch))
    path = str(tmp_path / "views.tfrecord")
    recs = [records.make_example([records.encode_png(u8[n, v]) for v in range(V)], n) for n in range(N)]
    records.write_tfrecords(path, recs)
    got, labels = next(iter(records.ViewBatcher(path, V, H, W, N, DEV, augment=False)))
    assert host(got).tobytes() == host(r.render(batch, quantize=True)).tobytes()
    assert labels.tolist() == [0, 1, 2]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def off_text(v, t):
    return "OFF\n%d %d 0\n" % (len(v), len(t)) + "".join("%r %r %r\n" % tuple(map(float, p)) for p in v) + \
        "".join("3 %d %d %d\n" % tuple(f) for f in t)


def test_render_modelnet_tool(tmp_path):
    src = tmp_path / "ModelNet"
    shapes = {"chair": [cube(), tetra()], "airplane": [R.icosphere(1)], "bed": [soup(12, 1)]}
    for cls, ms in shapes.items():
        d = src / cls / "train"
        d.mkdir(parents=True)
        for i, (v, t) in enumerate(ms):
            (d / ("%s_%04d.off" % (cls, i + 1))).write_text(off_text(v, t))
    (src / "chair" / "test").mkdir()
    out = str(tmp_path / "train.tfrecord")
    V, S = 3, 32
    _tool("render_modelnet").main(["--src", str(src), "--split", "train", "--out", out, "--views", str(V),
                                   "--size", str(S), "--batch", "2"])
    order = [("airplane", 0), ("bed", 0), ("chair", 0), ("chair", 1)]            # sorted classes, sorted files
    reloaded = [R.load_off(str(src / c / "train" / ("%s_%04d.off" % (c, i + 1)))) for c, i in order]
    want = host(R.ViewRenderer(V, S, S, device=DEV).render(reloaded))
    got, labels = next(iter(records.ViewBatcher(out, V, S, S, 4, DEV, augment=False)))
    assert host(got).tobytes() == want.tobytes()
    assert labels.tolist() == [0, 1, 2, 2]


# ---- engine integration --------------------------------------------------------------------------------------------
def make_engine(backbone, N, V, H, W, C, G, device=DEV, **kw):
    eng = gv.GVCNN(backbone, N, V, H, W, C, G, device=device, **kw)
    P = gv.params.init_backbone_params(eng.plan.param_shapes(), seed=2, perturb_bn=True)
    Hd = gv.params.init_head_params(V, eng.raw.c, eng.final.c, C, seed=3, spread_scores=True)
    eng.plan.bind(P)
    eng.set_head(Hd)
    return eng


@pytest.mark.parametrize("backbone,size,storage", [("resnet_v2_50", 64, "bf16"), ("inception_v3", 75, "f32")])
def test_forward_meshes_equals_forward(backbone, size, storage):
    N, V = 2, 3
    eng = make_engine(backbone, N, V, size, size, 10, 10, storage=storage)
    batch = R.MeshBatch([cube(), R.icosphere(2)], DEV)
    rots = R.random_rotations(N, "z", seed=1)
    r = R.ViewRenderer(V, size, size, device=DEV)
    got = [host(t).copy() for t in eng.forward_meshes(batch, rotations=rots)]
    views = r.render(batch, rotations=rots)
    want = [host(t).copy() for t in eng.forward(views)]
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    assert host(eng.forward_meshes(batch, renderer=r, rotations=rots)[2]).tobytes() == want[2].tobytes()
    with pytest.raises(ValueError):
        eng.forward_meshes(batch, renderer=R.ViewRenderer(V, size, size + 1, device=DEV))
    with pytest.raises(ValueError):
        eng.forward_meshes([cube()])


def test_embed_meshes_and_shape_index():
    N, V, S = 2, 3, 64
    eng = make_engine("resnet_v2_50", N, V, S, S, 10, 10, device="cuda", storage="bf16")     # the unindexed spelling
    r = R.ViewRenderer(V, S, S, device=DEV)
    groups = [[cube(), R.icosphere(1)], [tetra(), soup()]]
    idx_a, idx_b = gv.ShapeIndex(eng.final.c, device=DEV), gv.ShapeIndex(eng.final.c, device=DEV)
    for g in groups:
        idx_a.add(eng.embed_meshes(g))
        idx_b.add(eng.embed(r.render(g)))
    q = eng.embed_meshes(groups[0])
    da, ia = idx_a.search(q, k=4)
    db, ib = idx_b.search(q, k=4)
    assert host(ia).tolist() == host(ib).tolist()
    assert host(da).tobytes() == host(db).tobytes()
