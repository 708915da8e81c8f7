"""gvcnn-tf_amd — MI355X-native GVCNN hot path (per-view backbone + grouping module).

The directory name carries a hyphen (it is the name the build contract asks for); import it
as `gvcnn_tf_amd` through the shim module of that name at the repository root.

Importing this package loads libgvcnn_hip.so; a missing library is an ImportError — the HIP
library is the only compute path.
"""
from . import _lib

_lib.load()

from . import backbones, params  # noqa: E402
from . import model  # noqa: E402
from .model import (AUTO_REUSE, GVCNN, Explanation, basic, configure, explain_views, group_fusion,  # noqa: E402,F401
                    group_scheme, group_weight, grouping_module, gvcnn, gvcnn_fused, view_pooling)
from . import retrieval  # noqa: E402
from .retrieval import MetricLearner, ShapeIndex  # noqa: E402,F401
from . import render  # noqa: E402
from .render import (MeshBatch, PointBatch, ViewRenderer, estimate_normals, load_obj, load_off, load_points,  # noqa: E402,F401
                     pack_meshes, random_rotations, register, remove_outliers, sample_surface, voxel_downsample)

__all__ = ["GVCNN", "gvcnn", "basic", "group_scheme", "group_weight", "view_pooling", "group_fusion",
           "grouping_module", "gvcnn_fused", "configure", "explain_views", "Explanation", "AUTO_REUSE", "backbones", "params", "model", "retrieval",
           "ShapeIndex", "MetricLearner", "render", "MeshBatch", "ViewRenderer", "load_off", "load_obj", "pack_meshes",
           "random_rotations", "PointBatch", "load_points", "sample_surface", "estimate_normals", "remove_outliers",
           "voxel_downsample", "register"]
