"""The grouping head of both engines (model.GVCNN, training.TrainGVCNN): its buffers and its launch chain

    scorer responses -> view scores -> groups (+ status) -> view pooling + group fusion -> GAP -> Dense

(nets/model.py:144-164) on the device.  The steps are methods of their own because a sharded job puts a collective
between two of them (sharding.py); an engine on one device calls them in sequence.  Every step works on the head's own
buffers unless told otherwise, enqueues on the current stream and allocates nothing — the chain is captured into a
hipGraph — except `classify(num_shapes=...)`, which serves a batch of another size.
"""
import weakref

import torch

from . import _lib
from .backbones import _stream_ptr as _st

POOL_MODES = {"max": _lib.GV_VIEWPOOL_MAX, "mean": _lib.GV_VIEWPOOL_MEAN}


def raise_for_status(st, gidx, num_groups):
    """The status word of a group assignment as the exception the reference's numpy indexing raises."""
    if st & 2:
        raise ValueError("cannot convert float NaN to integer")
    if st & 1:
        bad = [int(b) for b in gidx.tolist() if b >= num_groups or b < 0]
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (bad[0], num_groups))


class GroupingHead:
    """Buffers (device tensors, fixed for the head's life):

        r_img        [N * own_views]  scorer responses of the engine's own views (a gathered set is passed in)
        scores gidx  [V]     scheme [G, V]     weight [G]         the grouping; per_shape: each with a leading [N]
        mean_scores  [V]     the batch-mean scores (`scores` itself unless per_shape)
        status       [1]     bit 1: a bin outside [0, G), bit 2: a NaN score
        S [N, h, w, C] (storage type)    gap [N, C]    logits [N, num_classes]
    """

    def __init__(self, engine, device, num_shapes, num_views, num_group, num_bins, final, num_classes, *, dtype, tdtype,
                 pool_mode, empty_fill, per_shape=False, weight_mode=_lib.GV_WEIGHT_COUNT, own_views=None):
        self._engine, self.device = weakref.proxy(engine), device
        self.N, self.V, self.G, self.num_bins = num_shapes, num_views, num_group, num_bins
        self.own_views = num_views if own_views is None else own_views
        self.h, self.w, self.c, self.num_classes = final.h, final.w, final.c, num_classes
        self.dtype, self.tdtype = dtype, tdtype
        self.pool_mode, self.empty_fill = pool_mode, float(empty_fill)
        self.per_shape, self.weight_mode = bool(per_shape), weight_mode
        f32, i32 = torch.float32, torch.int32
        lead = (num_shapes,) if self.per_shape else ()
        self.r_img = torch.empty(num_shapes * self.own_views, dtype=f32, device=device)
        self.scores = torch.empty(lead + (num_views,), dtype=f32, device=device)
        self.gidx = torch.empty(lead + (num_views,), dtype=i32, device=device)
        self.scheme = torch.empty(lead + (num_group, num_views), dtype=i32, device=device)
        self.weight = torch.empty(lead + (num_group,), dtype=f32, device=device)
        self.mean_scores = torch.empty(num_views, dtype=f32, device=device) if self.per_shape else self.scores
        self.status = torch.zeros(1, dtype=i32, device=device)
        self.S = torch.empty((num_shapes, final.h, final.w, final.c), dtype=tdtype, device=device)
        self.gap = torch.empty((num_shapes, final.c), dtype=f32, device=device)
        self.logits = torch.empty((num_shapes, num_classes), dtype=f32, device=device)

    @property
    def lib(self):
        return self._engine.lib                      # looked up per call: tools put a tracing proxy there

    def alias_onto(self, descriptor_name):
        """The buffers as attributes of the engine, under the names it has always shown them by: `scores` is the batch
        mean, the per-shape grouping carries `_ps`, the fused descriptor is `descriptor_name`."""
        ps = "_ps" if self.per_shape else ""
        names = dict(r_img="r_img", status="status", gap="gap", logits="logits", S=descriptor_name, mean_scores="scores",
                     scores="scores" + ps, gidx="gidx" + ps, scheme="scheme" + ps, weight="weight" + ps)
        for mine, theirs in names.items():
            setattr(self._engine, theirs, getattr(self, mine))

    # -- the chain ----------------------------------------------------------------------------------------------------
    def respond(self, raw_ptr, raw, score_kernel, score_bias):
        """r_img of the engine's own views from its raw tap (model.py:144-145); raw: the tap's tensor record."""
        _lib.check(self.lib.gv_view_score_partial(raw_ptr, raw.nb, raw.h * raw.w, raw.c, raw.ld, score_kernel.data_ptr(),
                                                  score_bias.data_ptr(), self.own_views, _lib.GV_ORDER_SHAPE_MAJOR,
                                                  self.r_img.data_ptr(), self.dtype, _st(None)),
                   "gv_view_score_partial")
        return self.r_img

    def finalize_scores(self, r_img=None, num_shapes=None, order=_lib.GV_ORDER_SHAPE_MAJOR):
        """mean_scores [V] from r_img (model.py:146-147); a shape-sharded job passes the responses of the global batch."""
        r_img = self.r_img if r_img is None else r_img
        _lib.check(self.lib.gv_view_score_finalize(r_img.data_ptr(), self.N if num_shapes is None else num_shapes, self.V,
                                                   order, self.mean_scores.data_ptr(), _st(None)),
                   "gv_view_score_finalize")
        return self.mean_scores

    def score(self, r_img=None):
        """The scores the groups are binned from: every shape's own (per_shape), else the batch mean."""
        if not self.per_shape:
            return self.finalize_scores(r_img)
        r_img = self.r_img if r_img is None else r_img
        _lib.check(self.lib.gv_view_score_per_shape(r_img.data_ptr(), self.N * self.V, self.scores.data_ptr(),
                                                    _st(None)), "gv_view_score_per_shape")
        return self.scores

    def assign(self, check=True):
        """scores -> gidx, scheme, weight and the status word (model.py:16-41)."""
        lib, st = self.lib, _st(None)
        out = (self.gidx.data_ptr(), self.scheme.data_ptr(), self.weight.data_ptr(), self.status.data_ptr())
        if self.per_shape:
            _lib.check(lib.gv_group_assign_per_shape(self.scores.data_ptr(), self.N, self.V, self.G, self.num_bins,
                                                     self.weight_mode, *out, st), "gv_group_assign_per_shape")
        else:
            _lib.check(lib.gv_group_assign(self.scores.data_ptr(), self.V, self.G, self.num_bins, *out, st),
                       "gv_group_assign")
        if check:
            self.check_status()
        return self.scheme, self.weight

    def check_status(self):
        """Raise what the reference raises for the last assignment (reads one int back: a sync)."""
        raise_for_status(int(self.status.item()), self.gidx.reshape(-1), self.G)

    def classify(self, F_ptr, cls_kernel, cls_bias, scheme=None, weight=None, num_shapes=None, pool_mode=None,
                 empty_fill=None):
        """View pooling + group fusion -> GAP -> Dense (model.py:154-164) over the descriptors at F_ptr
        ([N, V, h, w, C], storage type).  scheme [G', V] / weight [G'] (or [N, G', V] / [N, G']: per shape) default to
        the head's own.  num_shapes: F holds that many shapes and the results go to fresh tensors, not to S / gap /
        logits.  Returns (S, logits)."""
        lib, st = self.lib, _st(None)
        scheme = self.scheme if scheme is None else scheme
        weight = self.weight if weight is None else weight
        if num_shapes is None:
            N, S, gap, logits = self.N, self.S, self.gap, self.logits
        else:
            N = num_shapes
            S = torch.empty((N, self.h, self.w, self.c), dtype=self.tdtype, device=self.device)
            gap = torch.empty((N, self.c), dtype=torch.float32, device=self.device)
            logits = torch.empty((N, self.num_classes), dtype=torch.float32, device=self.device)
        E = self.h * self.w * self.c
        fuse, name = ((lib.gv_view_pool_fuse_fwd_per_shape, "gv_view_pool_fuse_fwd_per_shape") if scheme.dim() == 3
                      else (lib.gv_view_pool_fuse_fwd, "gv_view_pool_fuse_fwd"))
        _lib.check(fuse(F_ptr, self.V, N, E, E, self.V * E, scheme.data_ptr(), scheme.shape[-2], weight.data_ptr(),
                        self.pool_mode if pool_mode is None else pool_mode,
                        self.empty_fill if empty_fill is None else empty_fill, None, S.data_ptr(), self.dtype, st), name)
        _lib.check(lib.gv_global_avg_pool(S.data_ptr(), N, self.h * self.w, self.c, self.c, gap.data_ptr(), self.dtype,
                                          st), "gv_global_avg_pool")
        _lib.check(lib.gv_dense_fwd(gap.data_ptr(), N, self.c, cls_kernel.data_ptr(), cls_bias.data_ptr(),
                                    self.num_classes, logits.data_ptr(), st), "gv_dense_fwd")
        return S, logits
