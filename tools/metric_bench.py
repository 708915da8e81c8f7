"""Metric-learning timing: one MetricLearner.step (projection, all-pairs hinge loss / gradient, filter gradient, momentum
update) on one device, next to the same step written with torch.cdist + autograd on the same device and data.  One
JSON line per case.

    python tools/metric_bench.py [--window 0.5] [--warmup 3] [--no-profile]

Cases: (n, d, r) = (9843, 2048, 128) — the ModelNet40 training split as one batch — and (4096, 2048, 128), random
normal descriptors, 40 classes, calibrated so that the mean pair distance is 2 (b = 2).  The step is timed with device
events over at least `window` seconds of calls after `warmup` calls.  Per-kernel times come from one profiled call
(kernel durations summed by name; null when the profiler is unavailable); pair_tflops counts 4 n^2 rl for the pair
kernel alone, against the 157.3 TF/s fp32-MFMA peak.  loss_rel_diff compares the two losses of the first step.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gvcnn_tf_amd import retrieval as R  # noqa: E402

PEAK_TFLOPS_F32 = 157.3                        # MI355X fp32 MFMA
CASES = [("modelnet40_train", 9843, 2048, 128), ("batch4096", 4096, 2048, 128)]
KERNELS = ("project_kernel", "row_sqnorm_kernel", "pair_kernel", "pair_finish_kernel", "pair_stats_kernel",
           "wgrad_kernel", "wgrad_finish_kernel", "sgd_momentum")


def timed(fn, window, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    iters = max(5, int(math.ceil(window * 1000.0 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, iters


def kernel_ms(fn):
    """{kernel name: ms} of one call, from the profiler's device-kernel events; None if unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for key in sorted(KERNELS, key=len, reverse=True):     # "pair_finish_kernel" before "pair_kernel"
                if key in ev.name:
                    dt = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                    out[key] = out.get(key, 0.0) + dt / 1000.0
                    break
        return out or None
    except Exception:
        return None


class TorchStep:
    """The same objective and update in eager torch: cdist, the n x n hinge, autograd, momentum SGD."""

    def __init__(self, w, b, pos_weight):
        self.w = w.clone().requires_grad_(True)
        self.b = b.clone().requires_grad_(True)
        self.mw, self.mb = torch.zeros_like(w), torch.zeros_like(b)
        self.pw = pos_weight

    def __call__(self, x, lab, lr, mu):
        z = x @ self.w.t()
        d = torch.cdist(z, z).square()
        ok = lab >= 0
        up = torch.triu(ok[:, None] & ok[None, :], 1)
        pos = lab[:, None] == lab[None, :]
        y = torch.where(pos, 1.0, -1.0)
        c = torch.where(pos, self.pw, 1.0)
        loss = (c * torch.clamp(1.0 - y * (self.b - d), min=0.0) * up).sum() / up.sum()
        gw, gb = torch.autograd.grad(loss, (self.w, self.b))
        with torch.no_grad():
            self.mw.mul_(mu).add_(gw)
            self.mb.mul_(mu).add_(gb)
            self.w.sub_(lr * self.mw)
            self.b.sub_(lr * self.mb)
        return loss.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lr, mu = 0.01, 0.9
    for name, n, d, r in CASES:
        x = torch.randn(n, d, device=dev, generator=g)
        lab = torch.randint(0, 40, (n,), device=dev, generator=g)
        ml = R.MetricLearner(d, rank=r, seed=0, device=dev)
        ml.calibrate(x, lab)
        ts = TorchStep(ml.W.contiguous(), ml.b.reshape(()), ml.pos_weight)
        loss_dev = float(ml.loss_and_grads(x, lab)[0])
        loss_torch = float(ts(x, lab, 0.0, mu))
        _, stats = ml._pair(*ml._project(x), lab)
        stats = stats.cpu().numpy()
        step_ms, iters = timed(lambda: ml.step(x, lab, lr, mu), args.window, args.warmup)
        torch_ms, _ = timed(lambda: ts(x, lab, lr, mu), args.window, args.warmup)
        kms = None if args.no_profile else kernel_ms(lambda: ml.step(x, lab, lr, mu))
        pair_ms = kms.get("pair_kernel") if kms else None
        flop = 4.0 * n * n * ml.rl
        pair_tf = flop / (pair_ms * 1e-3) / 1e12 if pair_ms else None
        rec = {"case": name, "n": n, "d": d, "r": r, "rl": ml.rl, "pairs": int(stats[1]),
               "active_share_first_step": round(float(stats[2] / stats[1]), 4),
               "step_ms": round(step_ms, 4), "iters": iters,
               "kernel_ms": {k: round(v, 4) for k, v in kms.items()} if kms else None,
               "pair_tflops": round(pair_tf, 2) if pair_tf else None,
               "pair_peak_frac": round(pair_tf / PEAK_TFLOPS_F32, 4) if pair_tf else None,
               "torch_cdist_autograd_step_ms": round(torch_ms, 4),
               "speedup_vs_torch": round(torch_ms / step_ms, 2),
               "loss_rel_diff": abs(loss_dev - loss_torch) / abs(loss_torch)}
        print(json.dumps(rec), flush=True)
        del x, ts, ml
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
