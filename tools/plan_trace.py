#!/usr/bin/env python3
"""What the inference plan builder asks of the library, and the host state it leaves, as hashes: the check of a
host-side change to backbones.py against another commit.  A proxy in place of the loaded library records every
gv_plan_* call that backbones.make_plan issues, in order: integers, the bytes of descriptor arguments, null or non-null
for pointers, dependency arrays, the return code.  Per configuration it writes that list and its SHA-256, and the SHA-256
of the plan's state: filters, ss_specs, arena sizes, activation buffers, the vbuf -> physical map, (name, lane, deps) and
the whole record of every op, the end points, param_shapes(), total_flops, lanes_used.  On a device the list also holds
the gv_plan_run_range calls of declined_fused_pools (and a rebuilt plan's calls, where one was declined).  The same state
record, without native calls, is written for a TrainPlan of each backbone with fuse_siblings on and off.
Only the public surface of the package is used, so the same file runs against a checkout of an older commit.

    python tools/plan_trace.py --out DIR [--device cpu|cuda:0] [--root CHECKOUT]
    python tools/plan_trace.py --compare DIR_A DIR_B
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

SIZES = {"inception_v3": (139, (75, 128, 224)), "resnet_v2_50": (64, (97, 224))}       # default, the others
STORAGE = (("f32", "f32"), ("f32", "bf16x3"), ("bf16", "f32"), ("f16", "f32"))          # (storage, math; 16-bit: unused)
P3 = (("p3", True), ("p3all", "all"), ("nop3", False), ("p3set", ("Mixed_6b", "concat")))
SWITCHES = (("no_maxpool", dict(fuse_maxpool=False)), ("no_chain", dict(fuse_chain=False)), ("no_unit", dict(fuse_unit=False)),
            ("no_proj", dict(fuse_proj=False)), ("no_defer", dict(defer_preact=False)), ("unit_all", dict(fuse_unit="all")))
ENV_SWITCHES = ("GV_NO_CHAIN", "GV_NO_UNIT", "GV_UNIT_ALL", "GV_NO_PAIR", "GV_NO_POOL_ACT", "GV_NO_PROJ")
TAPS = (("tap2b", dict(raw_tap="Conv2d_2b_3x3")), ("early", dict(final_tap="Mixed_6a", raw_tap="Mixed_5d")))


def configs():
    """name -> (backbone, size, make_plan keywords).  Batch 2 everywhere."""
    out = {}
    for bb, (size, others) in SIZES.items():
        for st, math in STORAGE:
            base = dict(dtype=st, math=math)
            stem = "%s.%s-%s" % (bb, st, math if st == "f32" else "x")
            for lanes in (True, False):
                for pname, p3 in P3 if (st, math) == ("f32", "bf16x3") else P3[:1]:
                    out["%s.%s.lanes%d" % (stem, pname, lanes)] = (bb, size, dict(base, lanes=lanes, p3=p3))
            for name, kw in SWITCHES + (TAPS if bb == "inception_v3" else ()):
                out["%s.%s" % (stem, name)] = (bb, size, dict(base, **kw))
            for s in others:
                out["%s.size%d" % (stem, s)] = (bb, s, dict(base))
        for var in ENV_SWITCHES:                          # the whole-plan A/B switches of the environment, each set alone
            out["%s.bf16-x.env_%s" % (bb, var)] = (bb, size, dict(dtype="bf16", _env=var))
    return out


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":"), default=repr).encode()).hexdigest()


class TraceLib:
    """Stands where the loaded library stands: every gv_plan_* call with a status is recorded while `calls` is a list."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("gv_plan_") or fn.restype is not C.c_int:
            return fn

        def call(*args):
            rc = fn(*args)
            if self.calls is not None:
                types = list(fn.argtypes or ()) + [None] * len(args)
                row = []
                for k, (a, t) in enumerate(zip(args, types)):
                    obj = getattr(a, "_obj", None)                     # C.byref(structure)
                    if isinstance(obj, C.Structure):
                        row.append([type(obj).__name__, bytes(obj).hex()])
                    elif obj is not None:
                        row.append(type(obj).__name__)
                    elif isinstance(a, C.Array) and a._type_ is C.c_int32:      # a dependency list: its count follows
                        row.append([int(v) for v in a[:int(args[k + 1])]])
                    elif isinstance(a, C.Array) or (t is not None and issubclass(t, (C.c_void_p, C._Pointer))):
                        row.append("ptr" if a else "null")
                    elif t in (C.c_float, C.c_double):
                        row.append(float(a))
                    else:
                        row.append(None if a is None else int(a))
                self.calls.append([name, row, rc])
            return rc
        return call


def _state(p, native):
    ops = [{k: v for k, v in op.items()} for op in p.ops]
    st = dict(vbufs=[list(v) for v in p.vbufs],
              ops=[[op["name"], op.get("lane", 0), op.get("deps")] for op in p.ops], op_records=ops,
              end_points={k: repr(t) for k, t in p.end_points.items()}, end_point_order=list(p.end_points),
              param_shapes={k: list(v) for k, v in p.param_shapes().items()})
    if native:
        st.update(filters=[list(f) for f in p.filters], ss_specs=[list(s) for s in p.ss_specs], w_elems=p.w_elems,
                  ss_elems=p.ss_elems, act=[[list(t.shape), str(t.dtype)] for t in p.act], act_bytes=p.act_bytes,
                  vmap=sorted(p._phys.items()), total_flops=p.total_flops, lanes_used=p.lanes_used,
                  taps=[p.raw_tap, p.final_tap])
    return st


def trace(out, device):
    import torch
    from gvcnn_tf_amd import _lib, backbones
    from gvcnn_tf_amd.training import TrainPlan
    lib = TraceLib(_lib.load())
    _lib._lib = lib                                       # what _lib.load() hands out from here on
    summary = {}

    def emit(name, calls, state):
        rec = dict(calls=calls, state=state)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(rec, f, sort_keys=True, separators=(",", ":"), default=repr)
        summary[name] = dict(calls=len(calls), trace_sha256=_sha(calls), state_sha256=_sha(state))
        print("%-56s %4d calls  trace %s  state %s" % (name, len(calls), summary[name]["trace_sha256"][:16],
                                                       summary[name]["state_sha256"][:16]), flush=True)

    for name, (bb, size, kw) in configs().items():
        kw = dict(kw)
        var = kw.pop("_env", None)
        for v in ENV_SWITCHES:
            os.environ.pop(v, None)
        if var:
            os.environ[var] = "0"                         # ("set to anything" is what the switches test)
        lib.calls = []
        p = backbones.make_plan(bb, 2, size, size, torch.device(device), **kw)
        calls, lib.calls = lib.calls, None
        os.environ.pop(var or "", None)
        emit(name, calls, _state(p, True))
        del p
    for bb, (size, _) in SIZES.items():
        for fuse in (True, False) if bb == "inception_v3" else (None,):
            p = TrainPlan(2, size, size, backbones.MATH_MODES["bf16x3"])
            if bb == "inception_v3":
                backbones.build_inception_v3(p, keep=backbones.TAPS[bb], fuse_siblings=fuse)
            else:
                backbones.build_resnet_v2_50(p, keep=backbones.TAPS[bb])
            emit("train.%s%s" % (bb, "" if fuse is None else ".siblings%d" % fuse), [], _state(p, False))
    with open(os.path.join(out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
    n = len({(r["trace_sha256"], r["state_sha256"]) for r in summary.values()})
    print("%d configurations, %d distinct (trace, state) hashes, %d distinct trace hashes"
          % (len(summary), n, len({r["trace_sha256"] for r in summary.values()})))
    return 0


def compare(dir_a, dir_b):
    a, b = (json.load(open(os.path.join(d, "summary.json"))) for d in (dir_a, dir_b))
    bad = sorted(set(a) ^ set(b))
    for cfg in sorted(set(a) & set(b)):
        diff = [k for k in ("trace_sha256", "state_sha256") if a[cfg][k] != b[cfg][k]]
        if diff:
            bad.append(cfg)
            print("%-56s differs in %s (%d / %d calls)" % (cfg, ", ".join(diff), a[cfg]["calls"], b[cfg]["calls"]))
    print("%d configurations, %d distinct trace hashes in %s, %d differ%s" % (
        len(set(a) | set(b)), len({r["trace_sha256"] for r in a.values()}), dir_a, len(bad),
        ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is traced (default: this file's)")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    sys.path.insert(0, os.path.abspath(a.root))
    os.makedirs(a.out, exist_ok=True)
    return trace(a.out, a.device)


if __name__ == "__main__":
    sys.exit(main())
