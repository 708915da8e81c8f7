"""3D shape retrieval on GVCNN shape descriptors (the paper's second task next to classification).

    idx = ShapeIndex(2048, metric="l2", storage="bf16")
    idx.add(engine.embed(views), labels)
    dist, ids = idx.search(queries, k=10)          # k nearest stored shapes, on the device
    mAP = idx.self_map()                           # leave-one-out retrieval mAP (the ModelNet protocol)

The descriptor is `GVCNN.gap` ([N, C] fp32).  Rows are prepared once into the storage type (gv_retr_prepare), the
distances are an MFMA GEMM and the ranking (top-k, average precision over the full ranking) runs in
csrc/retrieval.hip; the order is (distance, row id) everywhere, so equal distances rank by the lower id.

    ml = MetricLearner(2048, rank=128)             # the paper's learned low-rank Mahalanobis metric (csrc/metric.hip)
    ml.fit(train_descriptors, train_labels, steps=200, lr=0.05)
    idx = ShapeIndex(2048, projection=ml)          # raw descriptors in, 128-wide projected rows stored and ranked
"""
import math
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
MAX_RANK = _lib.GV_METRIC_MAX_RANK
MAX_BATCH = _lib.GV_METRIC_MAX_BATCH


def _nanmean(ap):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # every query NaN -> NaN, without the warning
        return float(np.nanmean(ap.astype(np.float64)))


class ShapeIndex:
    """A growable index of shape descriptors [n, dim] with optional int64 labels (default -1: never relevant)."""

    def __init__(self, dim, metric="l2", storage="f32", device=None, projection=None):
        """projection: a MetricLearner over `dim`-wide descriptors.  add / search / average_precision then take raw
        descriptors, project them on the device, and the index stores and ranks `projection.rank`-wide rows."""
        if metric not in METRICS:
            raise ValueError("metric must be one of %s, not %r" % (sorted(METRICS), metric))
        if storage not in backbones.DTYPES:
            raise ValueError("storage must be one of %s, not %r" % (sorted(backbones.DTYPES), storage))
        if not isinstance(dim, (int, np.integer)) or dim <= 0:
            raise ValueError("dim must be a positive integer, not %r" % (dim,))
        if projection is not None:
            if not isinstance(projection, MetricLearner):
                raise ValueError("projection must be a MetricLearner, not %r" % (type(projection).__name__,))
            if projection.dim != dim:
                raise ValueError("the projection takes %d-wide descriptors, the index was given dim %d"
                                 % (projection.dim, dim))
        self.lib = _lib.load()
        self.projection = projection
        self.in_dim = int(dim)                                     # what add / search are fed
        self.dim = int(dim) if projection is None else projection.rank      # what is stored
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
        if x.dim() != 2 or x.shape[1] != self.in_dim:
            raise ValueError("%s must be [n, %d], got %s" % (what, self.in_dim, tuple(x.shape)))
        if not x.is_floating_point():
            x = x.to(torch.float32)
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if self.projection is not None and x.shape[0] > 0:
            x = self.projection.transform(x)
        return x

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

    def __init__(self, engine, metric="l2", storage="f32", projection=None):
        self.eng = engine
        self.index = ShapeIndex(engine.final.c, metric=metric, storage=storage, device=engine.device,
                                projection=projection)

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


class MetricLearner:
    """The paper's learned retrieval metric: a low-rank Mahalanobis projection z = W x (W [rank, dim] fp32) with a
    threshold b, trained on (descriptor, label) batches with the pairwise hinge loss over ALL pairs of the batch
    (Simonyan et al., Fisher Vector Faces in the Wild, 2013; the objective is written out in include/gvcnn_hip.h):

        L = (1/P) sum_{i<j} c_ij max(0, 1 - y_ij (b - |z_i - z_j|^2)),  c_ij = pos_weight for equal labels, 1 otherwise

    A label < 0 takes part in no pair.  Projection, the all-pairs loss / gradient (nothing n x n is materialised) and
    the filter gradient run in csrc/metric.hip on the exact fp32 MFMA with fixed-order reductions: the same inputs give
    the same bits every run.  W and b live in one flat buffer [rank * ld + 1] with a momentum buffer beside it; the
    update is gv_sgd_momentum on the W range (weight decay) and on the b element (none)."""

    def __init__(self, dim, rank=128, pos_weight=1.0, seed=0, device=None):
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or dim <= 0:
            raise ValueError("dim must be a positive integer, not %r" % (dim,))
        if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or not 1 <= rank <= MAX_RANK:
            raise ValueError("rank must be an integer in [1, %d], got %r" % (MAX_RANK, rank))
        if not (isinstance(pos_weight, (int, float)) and math.isfinite(pos_weight) and pos_weight > 0):
            raise ValueError("pos_weight must be a positive number, not %r" % (pos_weight,))
        self.dim, self.rank, self.pos_weight, self.seed = int(dim), int(rank), float(pos_weight), int(seed)
        self.ld = (self.dim + 3) // 4 * 4                          # row stride of W, of the gradient and of a batch
        self.rl = (self.rank + 63) // 64 * 64                      # row stride of Z
        self.lib = _lib.load()
        self.device = _model._dev(device)
        w = torch.randn((self.rank, self.dim), generator=torch.Generator().manual_seed(self.seed),
                        dtype=torch.float32) * (1.0 / math.sqrt(self.dim))       # N(0, 1/dim): the same bits everywhere
        nw = self.rank * self.ld
        self._p = torch.zeros(nw + 1, dtype=torch.float32, device=self.device)
        self._m = torch.zeros(nw + 1, dtype=torch.float32, device=self.device)
        self._g = torch.zeros(nw + 1, dtype=torch.float32, device=self.device)
        self._set(w.numpy(), 1.0)

    # -- parameters ---------------------------------------------------------------------------------------------
    @property
    def W(self):
        """[rank, dim] fp32 on the device (a view of the parameter buffer)."""
        return self._p[:-1].view(self.rank, self.ld)[:, :self.dim]

    @property
    def b(self):
        """The threshold: a 0-d fp32 view of the parameter buffer on the device."""
        return self._p[-1]

    def _flat(self, w, b):
        w = np.asarray(w, dtype=np.float32)
        if w.shape != (self.rank, self.dim):
            raise ValueError("W must be [%d, %d], got %s" % (self.rank, self.dim, w.shape))
        flat = np.zeros(self.rank * self.ld + 1, dtype=np.float32)
        flat[:-1].reshape(self.rank, self.ld)[:, :self.dim] = w
        flat[-1] = np.float32(b)
        return torch.from_numpy(flat)

    def _set(self, w, b):
        self._p.copy_(self._flat(w, b))

    def state_dict(self):
        p, m = self._p.cpu().numpy(), self._m.cpu().numpy()

        def cut(f):
            return f[:-1].reshape(self.rank, self.ld)[:, :self.dim].copy()
        return {"dim": self.dim, "rank": self.rank, "pos_weight": self.pos_weight, "W": cut(p), "b": p[-1].copy(),
                "momentum_W": cut(m), "momentum_b": m[-1].copy()}

    def load_state_dict(self, state):
        """W [rank, dim] and b (momentum_W / momentum_b optional: zero when absent)."""
        if state.get("dim", self.dim) != self.dim or state.get("rank", self.rank) != self.rank:
            raise ValueError("the state is for dim %r rank %r, this learner has dim %d rank %d"
                             % (state.get("dim"), state.get("rank"), self.dim, self.rank))
        p = self._flat(state["W"], state["b"])
        m = self._flat(state.get("momentum_W", np.zeros((self.rank, self.dim), np.float32)),
                       state.get("momentum_b", 0.0))
        self._p.copy_(p)
        self._m.copy_(m)
        self.pos_weight = float(state.get("pos_weight", self.pos_weight))
        return self

    # -- argument checks (no device needed) -----------------------------------------------------------------------
    def _check_rows(self, shape, what="descriptors"):
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError("%s must be [n, %d], got %s" % (what, self.dim, tuple(shape)))
        return int(shape[0])

    def _check_batch(self, shape, num_labels):
        n = self._check_rows(shape, "a batch")
        if n < 1 or n > MAX_BATCH:
            raise ValueError("a batch holds 1 to %d rows, got %d (fit(..., batch=) draws batches from more)"
                             % (MAX_BATCH, n))
        if num_labels != n:
            raise ValueError("labels must hold %d values, got %d" % (n, num_labels))
        return n

    def _rows(self, x, what="descriptors"):
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x))
        self._check_rows(x.shape, what)
        x = x.to(device=self.device, dtype=torch.float32)
        if self.ld != self.dim:
            x = torch.nn.functional.pad(x, (0, self.ld - self.dim))
        return x.contiguous()

    def _batch(self, x, labels):
        lab = torch.as_tensor(labels).reshape(-1)
        self._check_batch(tuple(x.shape) if hasattr(x, "shape") else np.shape(x), lab.numel())
        return self._rows(x, "a batch"), lab.to(device=self.device, dtype=torch.int64).contiguous()

    # -- the three kernels ----------------------------------------------------------------------------------------
    def _project(self, x):
        n = x.shape[0]
        z = torch.empty((n, self.rl), dtype=torch.float32, device=self.device)
        sq = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.gv_metric_project(x.data_ptr(), n, self.dim, self.ld, self._p.data_ptr(), self.rank,
                                              self.ld, z.data_ptr(), self.rl, sq.data_ptr(), _model._st()),
                   "gv_metric_project")
        return z, sq

    def _pair(self, z, sq, lab):
        n = z.shape[0]
        nb = self.lib.gv_metric_pair_workspace_bytes(n, self.rank)
        _lib.check(nb if nb < 0 else 0, "gv_metric_pair_workspace_bytes")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        dz = torch.empty((n, self.rl), dtype=torch.float32, device=self.device)
        stats = torch.empty(5, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gv_metric_pair_grad(z.data_ptr(), sq.data_ptr(), lab.data_ptr(), n, self.rank, self.rl,
                                                self._p.data_ptr() + 4 * self.rank * self.ld, self.pos_weight,
                                                dz.data_ptr(), stats.data_ptr(), ws.data_ptr(), nb, _model._st()),
                   "gv_metric_pair_grad")
        return dz, stats

    def _wgrad(self, dz, x, stats, loss):
        n = x.shape[0]
        nb = self.lib.gv_metric_wgrad_workspace_bytes(n, self.dim, self.rank)
        _lib.check(nb if nb < 0 else 0, "gv_metric_wgrad_workspace_bytes")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.gv_metric_wgrad(dz.data_ptr(), n, self.rank, self.rl, x.data_ptr(), self.dim, self.ld,
                                            stats.data_ptr(), self._g.data_ptr(), self.ld,
                                            None if loss is None else loss.data_ptr(), ws.data_ptr(), nb,
                                            _model._st()), "gv_metric_wgrad")

    def _grads(self, x, lab, loss):
        z, sq = self._project(x)
        dz, stats = self._pair(z, sq, lab)
        self._wgrad(dz, x, stats, loss)
        return z, dz, stats

    def _update(self, lr, mu, weight_decay):
        nw, st = self.rank * self.ld, _model._st()
        p, g, m = self._p.data_ptr(), self._g.data_ptr(), self._m.data_ptr()
        _lib.check(self.lib.gv_sgd_momentum(p, g, m, nw, lr, mu, weight_decay, st), "gv_sgd_momentum")
        _lib.check(self.lib.gv_sgd_momentum(p + 4 * nw, g + 4 * nw, m + 4 * nw, 1, lr, mu, 0.0, st),
                   "gv_sgd_momentum")

    # -- public ---------------------------------------------------------------------------------------------------
    def transform(self, descriptors):
        """z [n, rank] fp32 on the device (any n)."""
        with torch.cuda.device(self.device):
            x = self._rows(descriptors)
            if x.shape[0] == 0:
                return torch.empty((0, self.rank), dtype=torch.float32, device=self.device)
            z, _ = self._project(x)
            return z if self.rl == self.rank else z[:, :self.rank].contiguous()

    def pair_grad(self, x, labels):
        """The raw outputs of the pair kernel for one batch: (z [n, rank], dz_unnorm [n, rank] = 2 (s_i z_i - G_i), not
        divided by P, stats fp64 [5] = {sum c h, P, active pairs, sum a, sum d}), all on the device."""
        with torch.cuda.device(self.device):
            x, lab = self._batch(x, labels)
            z, sq = self._project(x)
            dz, stats = self._pair(z, sq, lab)
            return z[:, :self.rank], dz[:, :self.rank], stats

    def loss_and_grads(self, x, labels):
        """(loss, dL/dW [rank, dim], dL/db) of one batch on the device, normalised by P (all zero when P = 0)."""
        with torch.cuda.device(self.device):
            x, lab = self._batch(x, labels)
            loss = torch.empty(1, dtype=torch.float32, device=self.device)
            self._grads(x, lab, loss)
            g = self._g.clone()
            return loss[0], g[:-1].view(self.rank, self.ld)[:, :self.dim], g[-1]

    def step(self, x, labels, lr, mu=0.9, weight_decay=0.0, loss_out=None):
        """One momentum-SGD update on a batch [n <= MAX_BATCH, dim]; no synchronisation.  loss_out: a device fp32
        tensor of one element that receives the batch loss (before the update)."""
        with torch.cuda.device(self.device):
            x, lab = self._batch(x, labels)
            self._grads(x, lab, loss_out)
            self._update(float(lr), float(mu), float(weight_decay))

    def calibrate(self, x, labels):
        """Rescale W so that the mean pair distance of the batch is 2 and set b = 2 (one read-back).  Returns the
        mean pair distance before the rescaling."""
        with torch.cuda.device(self.device):
            x, lab = self._batch(x, labels)
            z, sq = self._project(x)
            _, stats = self._pair(z, sq, lab)
            st = stats.cpu().numpy()
            mean = float(st[4] / st[1]) if st[1] > 0 else 0.0
            if mean > 0.0:
                _lib.check(self.lib.gv_scale(self._p.data_ptr(), self.rank * self.ld, math.sqrt(2.0 / mean),
                                             _model._st()), "gv_scale")
            self._p[-1:].fill_(2.0)
            return mean

    def fit(self, descriptors, labels, steps, batch=None, lr=0.05, mu=0.9, weight_decay=0.0, calibrate=True):
        """calibrate (on the first batch) + `steps` updates.  batch None: every step sees all rows (at most MAX_BATCH);
        otherwise batches of `batch` rows walk seeded permutations of the rows.  Returns the loss of every step as
        numpy fp32 [steps] (one read-back at the end)."""
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError("steps must be a non-negative integer, not %r" % (steps,))
        if batch is not None and (isinstance(batch, bool) or not isinstance(batch, (int, np.integer))
                                  or not 1 <= batch <= MAX_BATCH):
            raise ValueError("batch must be an integer in [1, %d], got %r" % (MAX_BATCH, batch))
        with torch.cuda.device(self.device):
            lab = torch.as_tensor(labels).reshape(-1)
            x = descriptors if isinstance(descriptors, torch.Tensor) else torch.as_tensor(np.asarray(descriptors))
            n = self._check_rows(x.shape)
            if lab.numel() != n:
                raise ValueError("labels must hold %d values, got %d" % (n, lab.numel()))
            if batch is None or batch >= n:
                self._check_batch(x.shape, n)
                batch = None
            x = x.to(device=self.device, dtype=torch.float32)
            lab = lab.to(device=self.device, dtype=torch.int64)
            gen = torch.Generator().manual_seed(self.seed + 1)
            order, pos = None, 0

            def draw():
                nonlocal order, pos
                if batch is None:
                    return x, lab
                if order is None or pos + batch > n:
                    order, pos = torch.randperm(n, generator=gen).to(self.device), 0
                sel = order[pos:pos + batch]
                pos += batch
                return x[sel], lab[sel]

            hist = torch.zeros(max(int(steps), 1), dtype=torch.float32, device=self.device)
            for t in range(int(steps)):
                xb, lb = draw()
                if t == 0 and calibrate:
                    self.calibrate(xb, lb)
                self.step(xb, lb, lr, mu, weight_decay, loss_out=hist[t:t + 1])
            return hist[:int(steps)].cpu().numpy()
