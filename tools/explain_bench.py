"""Timing of the logit attribution (gv_explain_views) next to gv_view_pool_fuse_fwd on the same descriptors.

    python tools/explain_bench.py [--runs 20] [--no-engine]

Geometries: the final tap of BASELINE.json configs[1] (fp32, Inception-v3, 12 views of 224^2: 5 x 5 x 2048, 7 groups)
and configs[4] (f16, 20 views of 299^2: 8 x 8 x 2048, 10 groups), N = 32 shapes, F = max(0, normal), a random one-hot
scheme with count weights.  Each call is timed warm with device events, the median of `runs`; a call is everything the
entry point enqueues (for 'exact': the status reset, the target kernel, the map kernel, the finish).  The view-pool
forward reads the same bytes of F, so it is the yardstick; bytes/s counts F once for 'exact' and is given as a share of
the 6.3 TB/s a streaming kernel reaches on the MI355X (8 TB/s HBM3E peak).  Unless --no-engine: GVCNN.explain next to the
GVCNN.forward it contains, for the same two configurations.  One JSON line per case.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gvcnn_tf_amd as gv  # noqa: E402
from gvcnn_tf_amd import _lib  # noqa: E402

HBM_STREAM_TBS = 6.3
CASES = [("c1_f32_12x224", "f32", torch.float32, 12, 5, 2048, 7, "inception_v3", 224),
         ("c4_f16_20x299", "f16", torch.float16, 20, 8, 2048, 10, "inception_v3", 299)]
N = 32


def median_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def kernels(name, storage, td, V, hside, C, G, runs, dev):
    lib = _lib.load()
    code = {"f32": _lib.GV_F32, "bf16": _lib.GV_BF16, "f16": _lib.GV_F16}[storage]
    g = torch.Generator(device=dev).manual_seed(0)
    hw = hside * hside
    F = torch.randn(N, V, hw, C, device=dev, generator=g).clamp_(min=0).to(td).contiguous()
    rng = np.random.RandomState(0)
    s = np.zeros((G, V), dtype=np.int32)
    s[rng.randint(0, G, size=V), np.arange(V)] = 1
    scheme = torch.from_numpy(s).to(dev)
    weight = torch.from_numpy((1 + s.sum(1)).astype(np.float32)).to(dev)
    nc = 40
    K = torch.randn(C, nc, device=dev, generator=g) * 0.02
    b = torch.zeros(nc, device=dev)
    tg = torch.zeros(N, dtype=torch.int64, device=dev)
    E = hw * C
    S = torch.empty(N, E, dtype=td, device=dev)
    maps = torch.empty(N, V, hw, device=dev)
    contrib, base = torch.empty(N, V, device=dev), torch.empty(N, device=dev)
    tout, status = torch.empty(N, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gv_explain_workspace_bytes(V, N, C, 1) // 4, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        _lib.check(lib.gv_view_pool_fuse_fwd(F.data_ptr(), V, N, E, E, V * E, scheme.data_ptr(), G, weight.data_ptr(),
                                             0, 1.0, None, S.data_ptr(), code, st), "fwd")

    def explain(kind):
        _lib.check(lib.gv_explain_views(F.data_ptr(), V, N, hw, C, E, V * E, scheme.data_ptr(), G, weight.data_ptr(), 0, 0,
                                        1.0, K.data_ptr(), b.data_ptr(), nc, None, tg.data_ptr(), kind, maps.data_ptr(),
                                        contrib.data_ptr(), base.data_ptr(), tout.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), code, st), "explain")
    t_fwd = median_ms(fwd, runs)
    t_exact = median_ms(lambda: explain(0), runs)
    t_cam = median_ms(lambda: explain(1), runs)
    nbytes = F.numel() * F.element_size()
    tbs = nbytes / (t_exact * 1e-3) / 1e12
    return {"case": name, "what": "kernels", "N": N, "V": V, "hw": hw, "C": C, "G": G, "storage": storage,
            "F_MB": round(nbytes / 1e6, 1), "view_pool_fuse_fwd_ms": round(t_fwd, 4), "exact_ms": round(t_exact, 4),
            "gradcam_ms": round(t_cam, 4), "exact_over_fwd": round(t_exact / t_fwd, 2),
            "gradcam_over_fwd": round(t_cam / t_fwd, 2), "exact_TBps": round(tbs, 3),
            "exact_share_of_6.3TBps": round(tbs / HBM_STREAM_TBS, 3),
            "fwd_TBps": round(nbytes / (t_fwd * 1e-3) / 1e12, 3)}


def engine(name, storage, V, G, backbone, size, runs, dev):
    eng = gv.GVCNN(backbone, N, V, size, size, 40, G, device=dev, storage=storage, num_bins=G)
    x = torch.rand(N, V, size, size, 3, device=dev) - 0.5
    t_fwd = median_ms(lambda: eng.forward(x, check=False), runs, warmup=2)
    t_ex = median_ms(lambda: eng.explain(x, check=False), runs, warmup=2)
    t_cam = median_ms(lambda: eng.explain(x, kind="gradcam", check=False), runs, warmup=2)
    return {"case": name, "what": "engine", "forward_ms": round(t_fwd, 3), "explain_exact_ms": round(t_ex, 3),
            "explain_gradcam_ms": round(t_cam, 3), "exact_extra_over_forward": round(t_ex / t_fwd - 1.0, 4),
            "gradcam_extra_over_forward": round(t_cam / t_fwd - 1.0, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, storage, td, V, hside, C, G, backbone, size in CASES:
        print(json.dumps(kernels(name, storage, td, V, hside, C, G, args.runs, dev)), flush=True)
    if not args.no_engine:
        for name, storage, td, V, hside, C, G, backbone, size in CASES:
            print(json.dumps(engine(name, storage, V, G, backbone, size, max(5, args.runs // 4), dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
