"""Shape-retrieval timing: k-NN search (and, on the first case, leave-one-out AP) of ShapeIndex on one device, next to
torch.mm + torch.topk on the same device and data.  One JSON line per case.

    python tools/retrieval_bench.py [--iters 10] [--warmup 3] [--no-profile]

Cases: (nq, ndb, d) = (2468, 2468, 2048) — the ModelNet40 test set against itself — and (1024, 100000, 2048);
storage f32 / bf16; k 10 / 100.  Search and AP are timed with device events over `iters` calls after `warmup` calls,
on random normal descriptors.  The distance-GEMM and top-k kernels are timed separately from one profiled call (kernel
durations summed by name; null when the profiler is unavailable); gemm_tflops counts 2 * nq * ndb * ld.  Equality
with torch is checked on integer-valued descriptors of the same shapes (exact in every storage type): the same ids in
the same order (ties by id) and the same distances.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gvcnn_tf_amd import retrieval as R  # noqa: E402

# MI355X_MICROARCH.md: fp32 MFMA 157.3 TF/s; bf16 / f16 dense MFMA about 2.5 PF/s
PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "f16": 2500.0}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = [("modelnet40_test_self", 2468, 2468, 2048), ("db100k", 1024, 100000, 2048)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_ms(fn):
    """{kernel-name fragment: ms} of one call, from the profiler's device-kernel events; None if unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            name = ev.name
            for key in ("dist_gemm_kernel", "knn_select_kernel", "retr_ap_kernel"):
                if key in name:
                    dt = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                    out[key] = out.get(key, 0.0) + dt / 1000.0
        return out or None
    except Exception:
        return None


def torch_knn(q, x, k, dt):
    """torch reference: l2 distances through torch.mm in the storage type, then torch.topk (fp32)."""
    qs, xs = q.to(dt), x.to(dt)
    qn = (qs.float() ** 2).sum(1)
    xn = (xs.float() ** 2).sum(1)
    dots = torch.mm(qs, xs.t()).float()
    d = (qn[:, None] + xn[None, :] - 2.0 * dots).clamp_min_(0.0)
    return torch.topk(d, k, dim=1, largest=False, sorted=True)


def torch_exact_knn(q, x, k):
    """Integer inputs: exact distances in fp64, ties ordered by id through the key dist * ndb + id."""
    qd, xd = q.double(), x.double()
    d = ((qd ** 2).sum(1)[:, None] + (xd ** 2).sum(1)[None, :] - 2.0 * qd @ xd.t()).clamp_min_(0.0)
    key = d * x.shape[0] + torch.arange(x.shape[0], device=x.device, dtype=torch.float64)[None, :]
    _, ids = torch.topk(key, k, dim=1, largest=False, sorted=True)
    return torch.gather(d, 1, ids).float(), ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for ci, (name, nq, ndb, d) in enumerate(CASES):
        xr = torch.randn(ndb, d, device=dev, generator=g)
        qr = xr[:nq].clone() if nq == ndb else torch.randn(nq, d, device=dev, generator=g)
        xi = torch.randint(-3, 4, (ndb, d), device=dev, generator=g).float()
        qi = torch.randint(-3, 4, (nq, d), device=dev, generator=g).float()
        labels = torch.randint(0, 40, (ndb,), device=dev, generator=g)
        for storage in ("f32", "bf16"):
            idx = R.ShapeIndex(d, "l2", storage, device=dev).add(xr, labels)
            idx_i = R.ShapeIndex(d, "l2", storage, device=dev).add(xi)
            ld = idx.ld
            ap_ms = None
            if ci == 0:
                ap_ms = timed(lambda: idx.self_average_precision(), args.iters, args.warmup)
            for k in (10, 100):
                search_ms = timed(lambda: idx.search(qr, k), args.iters, args.warmup)
                torch_ms = timed(lambda: torch_knn(qr, xr, k, TORCH_DT[storage]), args.iters, args.warmup)
                kms = None if args.no_profile else kernel_ms(lambda: idx.search(qr, k))
                gemm_ms = kms.get("dist_gemm_kernel") if kms else None
                select_ms = kms.get("knn_select_kernel") if kms else None
                flop = 2.0 * nq * ndb * ld
                gemm_tf = flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms else None
                dd, di = idx_i.search(qi, k)
                td, ti = torch_exact_knn(qi, xi, k)
                equal = bool(torch.equal(di, ti) and torch.equal(dd, td))
                rec = {"case": name, "nq": nq, "ndb": ndb, "d": d, "storage": storage, "k": k,
                       "search_ms": round(search_ms, 4),
                       "ap_ms": round(ap_ms, 4) if ap_ms is not None and k == 10 else None,
                       "gemm_ms": round(gemm_ms, 4) if gemm_ms else None,
                       "select_ms": round(select_ms, 4) if select_ms else None,
                       "gemm_tflops": round(gemm_tf, 2) if gemm_tf else None,
                       "gemm_peak_frac": round(gemm_tf / PEAK_TFLOPS[storage], 4) if gemm_tf else None,
                       "search_tflops_e2e": round(flop / (search_ms * 1e-3) / 1e12, 2),
                       "torch_mm_topk_ms": round(torch_ms, 4),
                       "equal_to_torch_on_integer_inputs": equal}
                print(json.dumps(rec), flush=True)
            del idx, idx_i
        del xr, qr, xi, qi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
