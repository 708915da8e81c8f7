"""CPU checks of the learned retrieval metric: the two forms of the reference (tests/metric_ref.py) against each other
and against a hand-worked example, the new entry points' symbols, argument codes and workspace sizes, and the Python
layer's argument checks (no GPU)."""
import numpy as np
import pytest

import metric_ref as ref

BADARG, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                       # a 16-byte aligned stand-in pointer: never dereferenced here


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


# ---- the reference ------------------------------------------------------------------------------------------------
def test_reference_hand_worked():
    """Three points on a line (z = first coordinate: 0, 1, 2), labels 0 0 1, b = 1.5, pos_weight 2.
    (0,1) positive, d = 1: 1 - (1.5 - 1) = 0.5 > 0, active, c h = 1.   (1,2) negative, d = 1: 1 + (1.5 - 1) = 1.5, active.
    (0,2) negative, d = 4: 1 + (1.5 - 4) = -1.5, inactive.   L = (1 + 1.5) / 3.
    a_01 = 2, a_12 = -1: dL/dz = (2/3) (0 - 2, 1 + 2, -2 + 1) = (-4/3, 2, -2/3);  dL/db = -(2 - 1) / 3."""
    x = np.array([[0., 5.], [1., -1.], [2., 3.]])
    w = np.array([[1., 0.]])
    labels = [0, 0, 1]
    dz = np.array([-4 / 3, 2., -2 / 3])
    want = (2.5 / 3, np.array([[dz @ x[:, 0], dz @ x[:, 1]]]), -1 / 3)
    assert want[1][0, 0] == pytest.approx(2 / 3, abs=1e-15) and want[1][0, 1] == pytest.approx(-32 / 3, abs=1e-14)
    for f in (ref.loss_and_grads_closed, ref.loss_and_grads_autograd):
        loss, dw, db = f(x, w, 1.5, labels, 2.0)
        assert loss == pytest.approx(want[0], abs=1e-15)
        assert np.allclose(dw, want[1], rtol=0, atol=1e-14)
        assert db == pytest.approx(want[2], abs=1e-15)
    dz_un, stats = ref.pair_grad_closed(x @ w.T, labels, 1.5, 2.0)
    assert np.allclose(dz_un[:, 0] / 3, dz, rtol=0, atol=1e-15)
    assert stats.tolist() == [2.5, 3.0, 2.0, 1.0, 6.0]
    # the strict inequality: at b = 2 the positive pair sits exactly on the hinge and is not active
    _, stats = ref.pair_grad_closed(x @ w.T, labels, 2.0, 2.0)
    assert stats.tolist() == [2.0, 3.0, 1.0, -1.0, 6.0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_autograd_matches_closed_form(seed):
    rng = np.random.default_rng(seed)
    n, d, r = 60, 24, 5
    x = rng.normal(size=(n, d))
    w = rng.normal(size=(r, d)) / np.sqrt(d)
    labels = rng.integers(0, 4, size=n)
    labels[rng.random(n) < 0.1] = -1
    a = ref.loss_and_grads_closed(x, w, 1.7, labels, 1.5)
    b = ref.loss_and_grads_autograd(x, w, 1.7, labels, 1.5)
    assert a[0] > 0
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(a[1]).max()
    assert abs(a[2] - b[2]) <= 1e-12 * abs(a[2])


def test_reference_no_pairs():
    x = np.ones((3, 4))
    w = np.ones((2, 4))
    for labels in ([-1, -1, -1], [3, -1, -1]):
        for f in (ref.loss_and_grads_closed, ref.loss_and_grads_autograd):
            loss, dw, db = f(x, w, 1.0, labels, 1.0)
            assert loss == 0.0 and db == 0.0 and not np.asarray(dw).any()


# ---- C ABI ----------------------------------------------------------------------------------------------------------
NEW = ("gv_metric_project", "gv_metric_pair_workspace_bytes", "gv_metric_pair_grad", "gv_metric_wgrad_workspace_bytes",
       "gv_metric_wgrad")


def test_metric_symbols_and_constants(lib):
    import os
    from gvcnn_tf_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gvcnn_hip.h")).read()
    for n in NEW:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and (n + "(") in header
    assert "#define GV_METRIC_MAX_RANK 256" in header and "#define GV_METRIC_MAX_BATCH 16384" in header
    assert (_lib.GV_METRIC_MAX_RANK, _lib.GV_METRIC_MAX_BATCH) == (256, 16384)
    assert lib.gv_abi_version() == 1


def test_project_bad_arguments(lib):
    def call(x=P, n=10, d=100, x_ld=100, w=P, r=40, w_ld=100, z=P, rl=64, sq=P):
        return lib.gv_metric_project(x, n, d, x_ld, w, r, w_ld, z, rl, sq, None)
    for kw in ("x", "w", "z", "sq"):
        assert call(**{kw: None}) == BADARG, kw
    assert call(n=0) == BADARG and call(d=0) == BADARG and call(r=0) == BADARG and call(n=-2) == BADARG
    assert call(x_ld=96) == BADARG and call(w_ld=96) == BADARG            # row strides below d
    assert call(rl=40) == BADARG and call(rl=128) == BADARG               # rl is r rounded up to 64
    assert call(r=257, rl=320) == UNSUPPORTED
    assert call(x_ld=102) == ALIGN and call(w_ld=101) == ALIGN
    assert call(x=P + 4) == ALIGN and call(w=P + 8) == ALIGN and call(z=P + 4) == ALIGN


def test_pair_workspace_bytes(lib):
    f = lib.gv_metric_pair_workspace_bytes
    assert f(1, 1) > 0 and f(300, 16) > 0 and f(16384, 256) > 0
    assert f(300, 128) > f(300, 16)
    assert f(0, 16) == BADARG and f(10, 0) == BADARG and f(-1, 16) == BADARG
    assert f(16385, 16) == UNSUPPORTED and f(100, 257) == UNSUPPORTED
    for r in (16, 128, 256):                                              # linear in n
        assert f(16384, r) <= 4.1 * f(4096, r)
        assert f(8192, r) <= 4.1 * f(2048, r)


def test_pair_grad_bad_arguments(lib):
    ws_ok = lib.gv_metric_pair_workspace_bytes(100, 40)

    def call(z=P, sq=P, lab=P, n=100, r=40, rl=64, b=P, pw=1.0, dz=P, stats=P, ws=P, wsb=ws_ok):
        return lib.gv_metric_pair_grad(z, sq, lab, n, r, rl, b, pw, dz, stats, ws, wsb, None)
    for kw in ("z", "sq", "lab", "b", "dz", "stats", "ws"):
        assert call(**{kw: None}) == BADARG, kw
    assert call(n=0) == BADARG and call(r=0) == BADARG and call(rl=128) == BADARG and call(rl=40) == BADARG
    assert call(wsb=ws_ok - 1) == BADARG and call(wsb=0) == BADARG
    assert call(n=200) == BADARG                                          # the workspace was sized for 100 rows
    assert call(n=16385, wsb=1 << 40) == UNSUPPORTED and call(r=300, rl=320, wsb=1 << 40) == UNSUPPORTED
    assert call(z=P + 4) == ALIGN and call(dz=P + 8) == ALIGN and call(ws=P + 4) == ALIGN


def test_wgrad_bad_arguments(lib):
    f = lib.gv_metric_wgrad_workspace_bytes
    assert f(100, 70, 40) > 0 and f(16384, 2048, 256) > f(100, 2048, 256)
    assert f(0, 70, 40) == BADARG and f(100, 0, 40) == BADARG and f(100, 70, 0) == BADARG
    assert f(16385, 70, 40) == UNSUPPORTED and f(100, 70, 257) == UNSUPPORTED
    ws_ok = f(100, 70, 40)

    def call(dz=P, n=100, r=40, rl=64, x=P, d=70, x_ld=72, stats=P, grad=P, ld=72, loss=None, ws=P, wsb=ws_ok):
        return lib.gv_metric_wgrad(dz, n, r, rl, x, d, x_ld, stats, grad, ld, loss, ws, wsb, None)
    for kw in ("dz", "x", "stats", "grad", "ws"):
        assert call(**{kw: None}) == BADARG, kw
    assert call(n=0) == BADARG and call(d=0) == BADARG and call(r=0) == BADARG
    assert call(x_ld=64) == BADARG and call(rl=128) == BADARG
    assert call(ld=70) == BADARG and call(ld=76) == BADARG                # ld is d rounded up to 4
    assert call(wsb=ws_ok - 1) == BADARG
    assert call(n=16385, wsb=1 << 40) == UNSUPPORTED and call(r=257, rl=320, wsb=1 << 40) == UNSUPPORTED
    assert call(dz=P + 4) == ALIGN and call(ws=P + 8) == ALIGN


# ---- Python layer: argument errors before any launch ----------------------------------------------------------------
def test_metric_learner_rejects_bad_arguments(lib):
    import gvcnn_tf_amd
    from gvcnn_tf_amd import retrieval
    assert gvcnn_tf_amd.MetricLearner is retrieval.MetricLearner
    assert (retrieval.MAX_RANK, retrieval.MAX_BATCH) == (256, 16384)
    for rank in (0, 257, -1, 2.5, True):
        with pytest.raises(ValueError):
            retrieval.MetricLearner(64, rank=rank)
    for dim in (0, -3, 1.5):
        with pytest.raises(ValueError):
            retrieval.MetricLearner(dim)
    with pytest.raises(ValueError):
        retrieval.MetricLearner(64, pos_weight=0.0)
    ml = retrieval.MetricLearner.__new__(retrieval.MetricLearner)          # the batch checks need no device
    ml.dim, ml.rank = 64, 16
    assert ml._check_batch((100, 64), 100) == 100
    assert ml._check_batch((16384, 64), 16384) == 16384
    with pytest.raises(ValueError):
        ml._check_batch((16385, 64), 16385)                                # above MAX_BATCH
    with pytest.raises(ValueError):
        ml._check_batch((100, 64), 99)                                     # label count
    with pytest.raises(ValueError):
        ml._check_batch((100, 32), 100)                                    # wrong dim
    with pytest.raises(ValueError):
        ml._check_batch((100,), 100)
    with pytest.raises(ValueError):
        ml._check_batch((0, 64), 0)
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(32, projection=ml)                            # the projection takes 64-wide rows
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(64, projection=np.eye(64))                    # not a MetricLearner
