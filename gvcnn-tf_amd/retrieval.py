"""3D shape retrieval on GVCNN shape descriptors (the paper's second task next to classification).

    idx = ShapeIndex(2048, metric="l2", storage="bf16")
    idx.add(engine.embed(views), labels)
    dist, ids = idx.search(queries, k=10)          # k nearest stored shapes, on the device
    mAP = idx.self_map()                           # leave-one-out retrieval mAP (the ModelNet protocol)

The descriptor is `GVCNN.gap` ([N, C] fp32).  Rows are prepared once into the storage type (gv_retr_prepare), the
distances are an MFMA GEMM and the ranking (top-k, average precision over the full ranking) runs in
csrc/retrieval.hip; the order is (distance, row id) everywhere, so equal distances rank by the lower id.
"""
import warnings

import numpy as np
import torch

from . import _lib
from . import backbones
from . import model as _model

METRICS = {"l2": _lib.GV_METRIC_L2, "cosine": _lib.GV_METRIC_COSINE}
MAX_K = _lib.GV_KNN_MAX_K
AP_MAX_DB = _lib.GV_RETR_AP_MAX_NDB
DEFAULT_DB_CHUNK = 8192


def _nanmean(ap):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # every query NaN -> NaN, without the warning
        return float(np.nanmean(ap.astype(np.float64)))


class ShapeIndex:
    """A growable index of shape descriptors [n, dim] with optional int64 labels (default -1: never relevant)."""

    def __init__(self, dim, metric="l2", storage="f32", device=None):
        if metric not in METRICS:
            raise ValueError("metric must be one of %s, not %r" % (sorted(METRICS), metric))
        if storage not in backbones.DTYPES:
            raise ValueError("storage must be one of %s, not %r" % (sorted(backbones.DTYPES), storage))
        if not isinstance(dim, (int, np.integer)) or dim <= 0:
            raise ValueError("dim must be a positive integer, not %r" % (dim,))
        self.lib = _lib.load()
        self.dim = int(dim)
        self.metric_name, self.metric = metric, METRICS[metric]
        self.storage, self.dtype = storage, backbones.DTYPES[storage]
        self.tdtype = backbones.TORCH_DTYPES[self.dtype]
        self.ld = (self.dim + 63) // 64 * 64
        self.device = _model._dev(device)
        self._n = 0
        self._rows = torch.empty((0, self.ld), dtype=self.tdtype, device=self.device)
        self._sqnorm = torch.empty(0, dtype=torch.float32, device=self.device)
        self._labels = torch.empty(0, dtype=torch.int64, device=self.device)

    def __len__(self):
        return self._n

    @property
    def labels(self):
        return self._labels[:self._n]

    # -- preparation --------------------------------------------------------------------------------------------
    def _as_rows(self, x, what):
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x))
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError("%s must be [n, %d], got %s" % (what, self.dim, tuple(x.shape)))
        if not x.is_floating_point():
            x = x.to(torch.float32)
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _prepare(self, x, rows, sqnorm):
        n = x.shape[0]
        _lib.check(self.lib.gv_retr_prepare(x.data_ptr(), n, self.dim, self.dim, self.metric, self.dtype,
                                            rows.data_ptr(), self.ld, sqnorm.data_ptr(), _model._st()),
                   "gv_retr_prepare")

    def _prepare_queries(self, queries):
        x = self._as_rows(queries, "queries")
        nq = x.shape[0]
        if nq == 0:
            raise ValueError("no queries")
        rows = torch.empty((nq, self.ld), dtype=self.tdtype, device=self.device)
        sqn = torch.empty(nq, dtype=torch.float32, device=self.device)
        self._prepare(x, rows, sqn)
        return rows, sqn, nq

    def _exclude(self, exclude, nq):
        if exclude is None:
            return None
        e = torch.as_tensor(exclude).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if e.numel() != nq:
            raise ValueError("exclude must hold one row id per query (%d), got %d" % (nq, e.numel()))
        return e

    def add(self, descriptors, labels=None):
        """Append descriptors [n, dim] (float) with labels int64 [n] (None: -1).  Storage grows by doubling."""
        with torch.cuda.device(self.device):
            x = self._as_rows(descriptors, "descriptors")
            n = x.shape[0]
            if labels is None:
                lab = torch.full((n,), -1, dtype=torch.int64, device=self.device)
            else:
                lab = torch.as_tensor(labels).to(device=self.device, dtype=torch.int64).reshape(-1)
                if lab.numel() != n:
                    raise ValueError("labels must hold %d values, got %d" % (n, lab.numel()))
            if n == 0:
                return self
            need = self._n + n
            if need > self._rows.shape[0]:
                cap = max(need, 2 * self._rows.shape[0], 64)
                rows = torch.empty((cap, self.ld), dtype=self.tdtype, device=self.device)
                sqn = torch.empty(cap, dtype=torch.float32, device=self.device)
                labs = torch.empty(cap, dtype=torch.int64, device=self.device)
                rows[:self._n].copy_(self._rows[:self._n])
                sqn[:self._n].copy_(self._sqnorm[:self._n])
                labs[:self._n].copy_(self._labels[:self._n])
                self._rows, self._sqnorm, self._labels = rows, sqn, labs
            self._prepare(x, self._rows[self._n:need], self._sqnorm[self._n:need])
            self._labels[self._n:need].copy_(lab)
            self._n = need
        return self

    # -- search -------------------------------------------------------------------------------------------------
    def _check_k(self, k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
            raise ValueError("k must be an integer in [1, %d], got %r" % (MAX_K, k))
        return int(k)

    def search(self, queries, k, exclude=None, db_chunk=None):
        """(dist fp32 [nq, k], ids int64 [nq, k]) on the device, ascending by (distance, id); no synchronisation.
        A query with fewer than k candidates is padded with id -1 / distance +inf.  exclude [nq]: a row id to drop
        from each query's ranking (any value outside [0, len) drops nothing).  db_chunk: a multiple of 256 (speed
        only; the results are bitwise the same for every chunk size)."""
        k = self._check_k(k)
        if self._n == 0:
            raise ValueError("the index is empty")
        if db_chunk is None:
            db_chunk = min(DEFAULT_DB_CHUNK, (self._n + 255) // 256 * 256)
        if isinstance(db_chunk, bool) or not isinstance(db_chunk, (int, np.integer)) or db_chunk <= 0 \
                or db_chunk % 256:
            raise ValueError("db_chunk must be a positive multiple of 256, got %r" % (db_chunk,))
        with torch.cuda.device(self.device):
            q, qn, nq = self._prepare_queries(queries)
            return self._search(q, qn, nq, k, self._exclude(exclude, nq), int(db_chunk))

    def _search(self, q, qn, nq, k, exclude, db_chunk):
        lib = self.lib
        ws_bytes = lib.gv_knn_workspace_bytes(nq, db_chunk, k)
        _lib.check(ws_bytes if ws_bytes < 0 else 0, "gv_knn_workspace_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        _lib.check(lib.gv_knn_search(q.data_ptr(), qn.data_ptr(), nq, self._rows.data_ptr(), self._sqnorm.data_ptr(),
                                     self._n, self.dim, self.ld, self.metric, self.dtype, k,
                                     None if exclude is None else exclude.data_ptr(), db_chunk, dist.data_ptr(),
                                     ids.data_ptr(), ws.data_ptr(), ws_bytes, _model._st()), "gv_knn_search")
        return dist, ids

    # -- average precision --------------------------------------------------------------------------------------
    def _ap(self, q, qn, q_labels, nq, exclude):
        lib = self.lib
        if self._n == 0:
            raise ValueError("the index is empty")
        ws_bytes = lib.gv_retr_ap_workspace_bytes(nq, self._n)
        _lib.check(ws_bytes if ws_bytes < 0 else 0, "gv_retr_ap_workspace_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        ap = torch.empty(nq, dtype=torch.float32, device=self.device)
        _lib.check(lib.gv_retr_average_precision(q.data_ptr(), qn.data_ptr(), q_labels.data_ptr(), nq,
                                                 self._rows.data_ptr(), self._sqnorm.data_ptr(),
                                                 self._labels.data_ptr(), self._n, self.dim, self.ld, self.metric,
                                                 self.dtype, None if exclude is None else exclude.data_ptr(),
                                                 ap.data_ptr(), ws.data_ptr(), ws_bytes, _model._st()),
                   "gv_retr_average_precision")
        return ap

    def average_precision(self, queries, query_labels, exclude=None):
        """ap fp32 [nq] on the device: average precision of each query over the full ranking of the index (relevant:
        equal labels).  NaN for a query with a label < 0 or with no relevant stored shape.  len <= 16384."""
        with torch.cuda.device(self.device):
            q, qn, nq = self._prepare_queries(queries)
            lab = torch.as_tensor(query_labels).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            if lab.numel() != nq:
                raise ValueError("query_labels must hold %d values, got %d" % (nq, lab.numel()))
            return self._ap(q, qn, lab, nq, self._exclude(exclude, nq))

    def mean_average_precision(self, queries, query_labels, exclude=None):
        """The mean of average_precision over the queries that have one (nanmean), as a Python float (one read-back)."""
        return _nanmean(self.average_precision(queries, query_labels, exclude).cpu().numpy())

    def self_average_precision(self):
        """ap fp32 [len] on the device: every stored shape queries the others (leave-one-out)."""
        with torch.cuda.device(self.device):
            n = self._n
            ex = torch.arange(n, dtype=torch.int64, device=self.device)
            return self._ap(self._rows, self._sqnorm, self._labels, n, ex)

    def self_map(self):
        """Leave-one-out retrieval mAP with every stored shape as a query (the ModelNet protocol)."""
        return _nanmean(self.self_average_precision().cpu().numpy())


class RetrievalEvaluator:
    """Retrieval counterpart of evaluate.Evaluator: embed every batch with the engine, index it, report the
    leave-one-out mAP at the end."""

    def __init__(self, engine, metric="l2", storage="f32"):
        self.eng = engine
        self.index = ShapeIndex(engine.final.c, metric=metric, storage=storage, device=engine.device)

    def add_batch(self, views, labels, valid=None):
        """views [N,V,H,W,3], labels [N] (int64).  valid: the number of real shapes of a padded last batch (the
        Evaluator.add_batch convention); only those are indexed."""
        eng = self.eng
        v = eng.N if valid is None else int(valid)
        if not 0 <= v <= eng.N:
            raise ValueError("valid must be in [0, %d], got %d" % (eng.N, v))
        emb = eng.embed(views)
        lab = torch.as_tensor(labels).to(device=eng.device, dtype=torch.int64).reshape(-1)
        self.index.add(emb[:v], lab[:v])
        return v

    def result(self):
        """(mAP, per-query AP as numpy [num_shapes], num_shapes), leave-one-out over everything added."""
        ap = self.index.self_average_precision().cpu().numpy()
        return _nanmean(ap), ap, len(self.index)
