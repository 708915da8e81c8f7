#!/usr/bin/env python3
"""What a training step launches, and what it computes, as hashes: the check of a host-side change to the training
engine against another commit.  A proxy around eng.lib (steptime.TimedLib without the events) records, for two
consecutive train_step calls, every gv_* call in order: entry point, integer / float arguments, the bytes of ConvDesc /
PoolDesc arguments, the fields of a BnStats, null or non-null for every pointer, the return code.  Per configuration it
writes that list, its SHA-256, and the SHA-256 of loss, logits, every gradient and every parameter after the second step.
Only the engine's public surface and eng.lib are used, so the same file runs against a checkout of an older commit.

    python tools/train_launch_trace.py --out DIR [--config NAME ...] [--tune | --tiles FILE] [--dry]
    python tools/train_launch_trace.py --compare DIR_A DIR_B

--tune: one step, eng.autotune(), then the trace; the chosen table goes to DIR/tiles.json.  --tiles FILE installs such a
table instead of measuring, which takes the timing noise of the choice out of a comparison.  Without either no tile is
tuned, and a step (deterministic=True) repeats bit for bit across processes.  --dry answers every call with 0 instead
of launching it: the argument lists of the all-supported path, to be compared before anything new runs on a device."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BACKBONES = {"inception_v3": dict(num_shapes=2, num_views=3, height=139, width=139),
             "resnet_v2_50": dict(num_shapes=2, num_views=2, height=64, width=64)}
# name -> (constructor arguments, switches set on the engine)
VARIANTS = {
    "bf16": (dict(storage="bf16"), {}),
    "f32": (dict(storage="f32"), {}),
    "frozen_bn": (dict(storage="bf16", frozen_bn=True), {}),
    "scorer": (dict(storage="bf16", per_shape=True, weight_mode="mean_score", train_scorer=True), {}),
    "no_bn_stats": (dict(storage="bf16"), dict(fuse_bn_stats=False)),
    "no_bn_pool": (dict(storage="bf16"), dict(fuse_bn_pool=False)),
    "no_s2_classes": (dict(storage="bf16"), dict(s2_classes=False)),
    "no_pool_argmax": (dict(storage="bf16"), dict(pool_argmax=False)),
    "not_lazy": (dict(storage="bf16"), dict(_lazy=False)),
    # (the parity classes are chosen by size or by autotune: these maps are too small, so op["_s2_use"] is set)
    "s2_forced": (dict(storage="bf16"), dict(_s2_use=True)),
    "s2_concurrent": (dict(storage="bf16"), dict(_s2_use=True, s2_concurrent=True)),
}
CONFIGS = ["%s/%s" % (b, v) for b in BACKBONES for v in VARIANTS]
TILE_KEYS = ("tile_f", "tile_d", "tile_w", "_nofuse_f", "_nofuse_b", "_s2_use")


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _encode(arg, argtype):
    from gvcnn_tf_amd import _lib
    obj = getattr(arg, "_obj", None)                      # C.byref(structure)
    if isinstance(obj, (_lib.ConvDesc, _lib.PoolDesc)):
        return [type(obj).__name__, bytes(obj).hex()]
    if isinstance(obj, _lib.BnStats):
        return ["BnStats", obj.mode, obj.groups, obj.nseg,
                [[s.c0, s.c1, s.z_ld] + [bool(p) for p in (s.z, s.scale, s.shift, s.acc)] for s in obj.seg[:obj.nseg]]]
    if obj is not None:
        return type(obj).__name__
    if argtype in (C.c_float, C.c_double):
        return float(arg)
    if argtype is not None and issubclass(argtype, (C.c_void_p, C.c_char_p, C._Pointer)):
        return "ptr" if arg else "null"
    return None if arg is None else int(arg)


class TraceLib:
    """Wraps the loaded library: every gv_* call that returns a status is recorded while `calls` is a list."""

    def __init__(self, lib, dry=False):
        self._lib = lib
        self.calls = None
        self.dry = dry                                    # answer 0 without launching: the argument lists alone

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("gv_") or fn.restype is not C.c_int:
            return fn

        def call(*args):
            rc = 0 if self.dry else fn(*args)
            if self.calls is not None:
                types = list(fn.argtypes or ()) + [None] * len(args)
                self.calls.append([name, [_encode(a, t) for a, t in zip(args, types)], rc])
            return rc
        return call


def _tiles(eng):
    return [dict({k: op[k] for k in TILE_KEYS if k in op}, s2=[c["tile"] for c in op.get("s2", ())])
            for op in eng.plan.ops]


def _install(eng, table):
    assert len(table) == len(eng.plan.ops)
    for op, row in zip(eng.plan.ops, table):
        for k in TILE_KEYS:
            if k in row:
                op[k] = row[k]
        for c, t in zip(op.get("s2", ()), row["s2"]):
            c["tile"] = t


def run(config, out, tune=False, tiles=None, dry=False):
    import torch
    from gvcnn_tf_amd.training import TrainGVCNN
    backbone, variant = config.split("/")
    kwargs, switches = VARIANTS[variant]
    geo = BACKBONES[backbone]
    eng = TrainGVCNN(backbone, num_classes=40, num_group=10, device="cuda:0", **geo, **kwargs)
    for k, v in switches.items():
        if k == "_s2_use":
            for op in eng.plan.ops:
                if op.get("s2"):
                    op[k] = v
            continue
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(geo["num_shapes"], geo["num_views"], geo["height"], geo["width"], 3, generator=g) - 0.5).cuda()
    labels = torch.randint(0, 40, (geo["num_shapes"],), generator=g).cuda()
    table = None
    if tune or tiles is not None:
        eng.train_step(x, labels)                         # (autotune needs the buffers of one step; both sides take it,
        eng.repack()                                      # and the filter re-pack that autotune would start with)
        if tune:
            eng.autotune()
            table = _tiles(eng)
        else:
            _install(eng, tiles[config])
    eng.lib = lib = TraceLib(eng.lib, dry)
    lib.calls = []
    for _ in range(2):
        eng.train_step(x, labels)
    torch.cuda.synchronize()
    calls, lib.calls = lib.calls, None
    raw = lambda t: t.detach().cpu().contiguous().flatten().view(torch.uint8).numpy().tobytes()
    tensors = {} if dry else {"loss": _sha(raw(eng.loss)), "logits": _sha(raw(eng.logits))}
    for name, d in () if dry else (("grads", eng.grads), ("params", eng.params)):
        for k in sorted(d):
            tensors["%s[%s]" % (name, k)] = _sha(raw(d[k]))
    text = json.dumps(calls, separators=(",", ":"))
    stem = os.path.join(out, config.replace("/", "."))
    with open(stem + ".trace.json", "w") as f:
        f.write(text)
    res = dict(launches=len(calls), trace_sha256=_sha(text.encode()), loss=float(eng.loss), tensors_sha256=tensors,
               tensors_all_sha256=_sha(json.dumps(tensors, sort_keys=True).encode()))
    print("%-30s %5d launches  trace %s  tensors %s  loss %.6f" % (config, res["launches"], res["trace_sha256"][:16],
                                                                  res["tensors_all_sha256"][:16], res["loss"]), flush=True)
    return res, table


def compare(dir_a, dir_b):
    a, b = (json.load(open(os.path.join(d, "summary.json"))) for d in (dir_a, dir_b))
    bad = sorted(set(a) ^ set(b))
    for cfg in sorted(set(a) & set(b)):
        ra, rb = a[cfg], b[cfg]
        diff = [k for k in sorted(set(ra["tensors_sha256"]) | set(rb["tensors_sha256"]))
                if ra["tensors_sha256"].get(k) != rb["tensors_sha256"].get(k)]
        same = ra["trace_sha256"] == rb["trace_sha256"] and not diff
        print("%-30s %5d / %5d launches  trace %s %s %s  tensors %s %s %s (%d)" % (
            cfg, ra["launches"], rb["launches"], ra["trace_sha256"][:12], "==" if ra["trace_sha256"] == rb["trace_sha256"]
            else "!=", rb["trace_sha256"][:12], ra["tensors_all_sha256"][:12], "!=" if diff else "==",
            rb["tensors_all_sha256"][:12], len(ra["tensors_sha256"])))
        if not same:
            bad.append(cfg)
            for k in diff[:8]:
                print("    differs: " + k)
    print("%d configurations, %d differ%s" % (len(set(a) | set(b)), len(bad), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--config", action="append", choices=CONFIGS, help="default: all of them")
    ap.add_argument("--tune", action="store_true")
    ap.add_argument("--tiles")
    ap.add_argument("--dry", action="store_true", help="record the calls of the two steps without launching them")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    os.makedirs(a.out, exist_ok=True)
    tiles = json.load(open(a.tiles)) if a.tiles else None
    summary, tables = {}, {}
    for config in a.config or CONFIGS:
        summary[config], table = run(config, a.out, a.tune, tiles, a.dry)
        if table is not None:
            tables[config] = table
        with open(os.path.join(a.out, "summary.json"), "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)
    if tables:
        with open(os.path.join(a.out, "tiles.json"), "w") as f:
            json.dump(tables, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
