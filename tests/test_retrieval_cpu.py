"""CPU checks of the retrieval entry points: every bad argument returns its documented code before any HIP call, the
workspace sizes, the Python layer's argument checks, and the numpy oracle of average precision on hand-worked
rankings (the oracle test_gpu_retrieval.py compares the device with)."""
import math

import numpy as np
import pytest

BADARG, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                       # a 16-byte aligned stand-in pointer: never dereferenced here


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_library()
    import gvcnn_tf_amd
    return gvcnn_tf_amd._lib.load()


# ---- the numpy oracle ---------------------------------------------------------------------------------------------
def oracle_rank(dist_row, exclude=-1):
    """Row ids of one query's ranking: ascending distance, equal distances by the lower id; `exclude` dropped."""
    ids = np.arange(len(dist_row))
    order = np.lexsort((ids, dist_row))
    return order[order != exclude]


def oracle_ap(dist_row, q_label, db_labels, exclude=-1):
    """AP = (1/R) sum_j j / rank_j over the full ranking; NaN for q_label < 0 or R == 0."""
    if q_label < 0:
        return float("nan")
    rel = np.asarray(db_labels)[oracle_rank(dist_row, exclude)] == q_label
    R = int(rel.sum())
    if R == 0:
        return float("nan")
    ranks = np.nonzero(rel)[0] + 1
    return float(np.sum(np.arange(1, R + 1) / ranks) / R)


def test_oracle_ap_hand_worked():
    # relevant / irrelevant / relevant: (1/1 + 2/3) / 2
    assert oracle_ap(np.array([0., 1., 2.]), 7, [7, 3, 7]) == pytest.approx((1 + 2 / 3) / 2, abs=1e-15)
    # ties rank by id: rows 1 and 0 at the same distance -> 0 first (irrelevant), then 1 (relevant): 1/2
    assert oracle_ap(np.array([5., 5.]), 1, [0, 1]) == pytest.approx(0.5, abs=1e-15)
    # excluding the only relevant row, a query label < 0, a database label < 0 never relevant
    assert math.isnan(oracle_ap(np.array([0., 1.]), 2, [2, 0], exclude=0))
    assert math.isnan(oracle_ap(np.array([0., 1.]), -1, [-1, -1]))
    assert oracle_ap(np.array([0., 1., 2.]), 4, [-1, 4, 9], exclude=0) == pytest.approx(1.0, abs=1e-15)
    assert list(oracle_rank(np.array([3., 1., 3., 0.]), exclude=1)) == [3, 0, 2]


# ---- C ABI argument checks ------------------------------------------------------------------------------------------
def test_retrieval_symbols_and_constants(lib):
    from gvcnn_tf_amd import _lib
    for n in ("gv_retr_prepare", "gv_knn_workspace_bytes", "gv_knn_search", "gv_retr_ap_workspace_bytes",
              "gv_retr_average_precision"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert (_lib.GV_METRIC_L2, _lib.GV_METRIC_COSINE, _lib.GV_KNN_MAX_K) == (0, 1, 256)
    assert lib.gv_abi_version() == 1


def test_prepare_bad_arguments(lib):
    def call(x=P, n=4, d=100, x_ld=100, metric=0, dtype=0, y=P, ld=128, sq=P):
        return lib.gv_retr_prepare(x, n, d, x_ld, metric, dtype, y, ld, sq, None)
    assert call(x=None) == BADARG
    assert call(y=None) == BADARG
    assert call(sq=None) == BADARG
    assert call(n=0) == BADARG and call(d=0) == BADARG and call(n=-3) == BADARG
    assert call(x_ld=99) == BADARG                 # row stride below d
    assert call(ld=64) == BADARG                   # storage row shorter than d
    assert call(metric=2) == BADARG and call(metric=-1) == BADARG
    assert call(dtype=3) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(ld=160) == ALIGN                   # not a multiple of 64
    assert call(y=P + 8) == ALIGN                  # storage pointer not 16-byte aligned


def test_knn_workspace_bytes(lib):
    f = lib.gv_knn_workspace_bytes
    base = f(100, 256, 10)
    assert base > 0
    assert f(200, 256, 10) > base and f(100, 512, 10) > base and f(100, 256, 20) > base
    assert f(100, 256, 256) > 0
    assert f(0, 256, 10) == BADARG and f(100, 0, 10) == BADARG and f(100, 100, 10) == BADARG
    assert f(100, -256, 10) == BADARG and f(100, 256, 0) == BADARG and f(100, 256, 257) == BADARG


def test_ap_workspace_bytes(lib):
    f = lib.gv_retr_ap_workspace_bytes
    base = f(100, 1000)
    assert base > 0
    assert f(200, 1000) > base and f(100, 2000) > base
    assert f(1, 16384) > 0
    assert f(0, 10) == BADARG and f(10, 0) == BADARG
    assert f(10, 16385) == UNSUPPORTED


def test_knn_search_bad_arguments(lib):
    ws_ok = lib.gv_knn_workspace_bytes(8, 256, 10)

    def call(q=P, qn=P, nq=8, db=P, dbn=P, ndb=50, d=100, ld=128, metric=0, dtype=0, k=10, ex=None, chunk=256,
             dist=P, idx=P, ws=P, wsb=ws_ok):
        return lib.gv_knn_search(q, qn, nq, db, dbn, ndb, d, ld, metric, dtype, k, ex, chunk, dist, idx, ws, wsb,
                                 None)
    for kw in ("q", "qn", "db", "dbn", "dist", "idx", "ws"):
        assert call(**{kw: None}) == BADARG, kw
    assert call(nq=0) == BADARG and call(ndb=0) == BADARG and call(d=0) == BADARG and call(d=-5) == BADARG
    assert call(ld=64) == BADARG                   # ld < d
    assert call(k=0) == BADARG and call(k=257) == BADARG and call(k=-1) == BADARG
    assert call(metric=5) == BADARG
    assert call(chunk=0) == BADARG and call(chunk=100) == BADARG and call(chunk=-256) == BADARG
    assert call(wsb=ws_ok - 1) == BADARG and call(wsb=0) == BADARG
    assert call(k=20) == BADARG                    # the workspace was sized for k = 10
    assert call(dtype=3) == UNSUPPORTED
    assert call(ld=160) == ALIGN
    assert call(q=P + 4) == ALIGN and call(db=P + 2) == ALIGN and call(ws=P + 8) == ALIGN


def test_ap_bad_arguments(lib):
    ws_ok = lib.gv_retr_ap_workspace_bytes(8, 50)

    def call(q=P, qn=P, ql=P, nq=8, db=P, dbn=P, dbl=P, ndb=50, d=100, ld=128, metric=0, dtype=0, ex=None, ap=P,
             ws=P, wsb=ws_ok):
        return lib.gv_retr_average_precision(q, qn, ql, nq, db, dbn, dbl, ndb, d, ld, metric, dtype, ex, ap, ws, wsb,
                                             None)
    for kw in ("q", "qn", "ql", "db", "dbn", "dbl", "ap", "ws"):
        assert call(**{kw: None}) == BADARG, kw
    assert call(nq=0) == BADARG and call(ndb=-1) == BADARG and call(d=0) == BADARG and call(ld=64) == BADARG
    assert call(metric=2) == BADARG
    assert call(wsb=ws_ok - 1) == BADARG and call(ndb=100) == BADARG     # workspace sized for 50 rows
    assert call(dtype=7) == UNSUPPORTED
    assert call(ndb=16385, wsb=1 << 40) == UNSUPPORTED                    # above the documented cap
    assert call(ld=100) == ALIGN
    assert call(q=P + 8) == ALIGN and call(db=P + 4) == ALIGN and call(ws=P + 2) == ALIGN


# ---- Python layer: argument errors before any launch ----------------------------------------------------------------
def test_shape_index_rejects_bad_configuration(lib):
    from gvcnn_tf_amd import retrieval
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(2048, metric="euclid")
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(2048, storage="f64")
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(0)
    with pytest.raises(ValueError):
        retrieval.ShapeIndex(-4)
    idx = retrieval.ShapeIndex.__new__(retrieval.ShapeIndex)           # the k check needs no device
    for k in (0, 257, -1, 2.5, True):
        with pytest.raises(ValueError):
            idx._check_k(k)
    assert idx._check_k(256) == 256
    import gvcnn_tf_amd
    assert gvcnn_tf_amd.ShapeIndex is retrieval.ShapeIndex
