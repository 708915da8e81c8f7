#!/usr/bin/env python3
"""Training-step throughput (--storage f32: fp32 storage, bf16x3 math; bf16: 16-bit storage and MFMA): forward(train BN) + loss + backward + Momentum.
    python tools/train_bench.py [--backbone inception_v3] [--shapes 8] [--views 12] [--size 224]
--per-shape --weight-mode mean_score [--train-scorer]: the paper's grouping head, with the scorer's gradient; the
backward time is split into head and trunk, and with --train-scorer the two scorer entry points are timed on their own."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gvcnn_tf_amd.training import TrainGVCNN

ap = argparse.ArgumentParser()
ap.add_argument("--backbone", default="inception_v3")
ap.add_argument("--shapes", type=int, default=8)
ap.add_argument("--views", type=int, default=12)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--storage", default="f32", choices=["f32", "bf16", "f16"])
ap.add_argument("--graph", action="store_true", help="replay the whole step from one captured graph")
ap.add_argument("--lanes", action="store_true", help="branches of a block on separate streams (meant for --graph)")
ap.add_argument("--per-shape", action="store_true", help="per-shape grouping (the paper's module)")
ap.add_argument("--weight-mode", default="count", choices=["count", "mean_score"])
ap.add_argument("--train-scorer", action="store_true", help="scorer gradients through the mean_score group weights")
a = ap.parse_args()
eng = TrainGVCNN(a.backbone, a.shapes, a.views, a.size, a.size, 40, 10, device="cuda:0", storage=a.storage,
                 per_shape=a.per_shape, weight_mode=a.weight_mode, train_scorer=a.train_scorer)
x = (torch.rand(a.shapes, a.views, a.size, a.size, 3) - 0.5).cuda()
labels = torch.randint(0, 40, (a.shapes,)).cuda()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
ap_tune = os.environ.get("GV_NO_TUNE") is None
eng.train_step(x, labels, lr=1e-6)
if ap_tune:
    eng.autotune()              # untimed: per-launch tile choice (speed only)
    eng.train_step(x, labels, lr=1e-6)
torch.cuda.synchronize()
tf = tb = to = th = 0.0
for _ in range(a.steps):
    ev[0].record(); eng.forward(x, labels, check=False); ev[1].record()
    eng.backward_head(); ev[4].record(); eng.backward_backbone(); ev[2].record()      # (= eng.backward())
    eng.apply_momentum(1e-6); eng.repack(); ev[3].record(); torch.cuda.synchronize()
    tf += ev[0].elapsed_time(ev[1]); tb += ev[1].elapsed_time(ev[2]); to += ev[2].elapsed_time(ev[3])
    th += ev[1].elapsed_time(ev[4])
if a.lanes:
    eng.enable_lanes()
    eng.train_step(x, labels, lr=1e-6)
    torch.cuda.synchronize()
if a.graph:
    # the whole step (forward, loss, backward, moving averages, Momentum, filter re-pack) as ONE graph launch
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        eng.train_step(x, labels, lr=1e-6); eng.repack()
    torch.cuda.current_stream().wait_stream(s_)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        eng.forward(x, labels, check=False); eng.backward(); eng.update_moving_averages(); eng.apply_momentum(1e-6); eng.repack(sync=False)
    gr.replay(); torch.cuda.synchronize()
    ev[0].record()
    for _ in range(a.steps):
        gr.replay()
    ev[1].record(); torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / a.steps
    print("[%s] graph replay: %.2f ms/step => %.1f views/s (loss %.4f)" % (a.storage, ms, a.shapes * a.views / (ms * 1e-3), float(eng.loss)))
n = a.steps
if a.per_shape:                                   # (the default invocation prints what it always printed)
    print("[%s] head backward %.3f ms of the backward pass (per_shape=%d weight_mode=%s train_scorer=%d)"
          % (a.storage, th / n, a.per_shape, a.weight_mode, a.train_scorer))
if a.train_scorer:
    # the two scorer entry points on their own, on the engine's buffers (both store: repeating them changes nothing)
    from gvcnn_tf_amd import _lib
    from gvcnn_tf_amd.model import _st
    f, r, V = eng.final, eng.raw, eng.V
    E = f.h * f.w * f.c
    nk = eng.score_kernel.numel()
    calls = {
        "gv_group_weight_bwd_per_shape": lambda: eng.lib.gv_group_weight_bwd_per_shape(
            eng._ptr(f), eng.dS.data_ptr(), V, eng.N, E, E, V * E, eng.scheme_ps.data_ptr(), eng.G,
            eng.weight_ps.data_ptr(), eng.pool_mode, eng.dw_ps.data_ptr(), eng._gw_ws.data_ptr(), eng._gw_ws.numel(),
            eng.dt, _st()),
        "gv_view_score_bwd": lambda: eng.lib.gv_view_score_bwd(
            eng._ptr(r), r.nb, r.h * r.w, r.c, r.ld, eng.score_kernel.data_ptr(), eng.r_img.data_ptr(),
            eng.gidx_ps.data_ptr(), eng.dw_ps.data_ptr(), eng.G, V, eng._flat_sg.data_ptr(),
            eng._flat_sg.data_ptr() + 4 * nk, eng._ptr(r, grad=True), r.ld, 0, eng.dt, _st()),
    }
    reps = 20
    for name, fn in calls.items():
        _lib.check(fn(), name)
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record(); torch.cuda.synchronize()
        print("[%s] %s: %.1f us (F %.1f MB, raw tap %.1f MB)" % (a.storage, name, ev[0].elapsed_time(ev[1]) / reps * 1e3,
              eng.N * V * E * eng.es / 1e6, r.nb * r.h * r.w * r.c * eng.es / 1e6))
flops = sum(op.get("flops", 0) for op in eng.plan.ops)
print("[%s] " % a.storage + "%s %dx%d views %d^2: forward %.2f ms, backward %.2f ms, update+repack %.2f ms => %.1f views/s; fwd %.1f TF/s, bwd(2x flops) %.1f TF/s"
      % (a.backbone, a.shapes, a.views, a.size, tf / n, tb / n, to / n, a.shapes * a.views / ((tf + tb + to) / n * 1e-3),
         flops / (tf / n) / 1e9, 2 * flops / (tb / n) / 1e9))
