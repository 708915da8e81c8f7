#!/usr/bin/env python3
"""Per-layer time of the filter gradient on the training geometry: the fp32 MFMA; on 16-bit storage the fp32 MFMA with
typed loads beside the 16-bit MFMA kernels.
    python tools/wgrad_times.py [--shapes 32]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gvcnn_tf_amd import _lib  # noqa: E402
from gvcnn_tf_amd.training import TrainGVCNN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=int, default=32)
ap.add_argument("--backbone", default="inception_v3")
ap.add_argument("--storage", default="f32")
a = ap.parse_args()
dev = torch.device("cuda:0")
eng = TrainGVCNN(a.backbone, a.shapes, 12, 224, 224, 40, 7, device=dev, num_bins=7, storage=a.storage)
lib = _lib.load()
x = (torch.rand(a.shapes, 12, 224, 224, 3, device=dev) - 0.5)
eng.forward(x, torch.zeros(a.shapes, dtype=torch.int64), check=False)
eng.backward()
torch.cuda.synchronize()
st = torch.cuda.current_stream().cuda_stream
forms = ["f32 mfma"] if a.storage == "f32" else ["f32 mfma", "16-bit mfma"]
tot = [0.0] * len(forms)
for op in eng.plan.ops:
    if op["kind"] != "conv":
        continue
    xx, y = op["x"], op["y"]
    d = eng._conv_desc(op)
    dw = eng._dw(op)
    res = []
    for form in forms:
        lib.gv_conv2d_wgrad_set_lp_f32(1 if a.storage != "f32" and form == "f32 mfma" else 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lib.gv_conv2d_wgrad(C.byref(d), eng._ptr(xx), eng._ptr(y, True), y.ld, dw.data_ptr(), st)
        e0.record()
        for _ in range(3):
            lib.gv_conv2d_wgrad(C.byref(d), eng._ptr(xx), eng._ptr(y, True), y.ld, dw.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 3)
    lib.gv_conv2d_wgrad_set_lp_f32(0)
    tot = [t + r for t, r in zip(tot, res)]
    fl = op["flops"]
    print("%-55s M=%8d cin=%4d cout=%4d k=%dx%d" % (op["name"][-55:], y.npix, xx.c, y.c, op["kh"], op["kw"]) +
          "".join("  %s %7.3f ms %6.1f TF" % (f, r, fl / r / 1e9) for f, r in zip(forms, res)))
print("total " + ", ".join("%s %.2f ms" % (f, t) for f, t in zip(forms, tot)))
