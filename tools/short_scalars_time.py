"""Device time of amdmsm_msm_device_short against the only route a caller had before it: the same values widened to Fr
records through amdmsm_msm_device.  Device-resident inputs, median and minimum of the repetitions after a warm-up, phase
times from amdmsm_get_timings.

    python tools/short_scalars_time.py                         # table 1: old route against new, U8 / U32 / U64
    python tools/short_scalars_time.py --old tools/old_libamdmsm.so
                                                               # the old route timed on the parent commit's library
    python tools/short_scalars_time.py --sweep                 # table 2: forced c = 6 .. 16 against the planner's choice
    python tools/short_scalars_time.py --host                  # table 3: host entry, U32 against widened Fr, bases registered

The parent's library is built from a checkout of the parent commit (python -m libff_amd.build there) and copied to
tools/old_libamdmsm.so, as for tools/ab_fixed_base.py; it is loaded in a child process of its own (AMDMSM_LIBRARY).
Raw output: profiles/short_scalars.txt.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"alt_bn128_g1": (0, 1), "bls12_377_g1": (1, 1)}
KINDS = {"u8": (1, np.uint8), "u32": (4, np.uint32), "u64": (8, np.uint64)}
PHASES = ("clear", "sort", "accumulate", "reduce", "final", "total")


def widen(v, fl):
    out = np.zeros((len(v), fl), dtype=np.uint64)
    out[:, 0] = v
    return out


class Bench:
    def __init__(self, curve, group, n):
        import libff_amd

        self.la = libff_amd
        self.e = libff_amd.Engine(0)
        self.curve, self.group, self.n = curve, group, n
        s = libff_amd.sizes(curve, group)
        self.s = s
        self.d_aff = self.e.malloc(n * s["affine_bytes"])
        self.e.gen_bases_seq_device(curve, group, 0, n, self.d_aff)
        self.d_sc = self.e.malloc(n * s["fr_bytes"])
        self.d_out = self.e.malloc(s["g_bytes"])
        self.e.set_timing(True)

    def time(self, call, reps, warmup):
        for _ in range(warmup):
            call()
        self.e.synchronize()
        tot, phases = [], []
        for _ in range(reps):
            call()
            ms = self.e.get_timings()
            tot.append(ms[5])
            phases.append(ms[:6])
        med = statistics.median(tot)
        ph = [statistics.median(p[i] for p in phases) for i in range(6)]
        return {"median_ms": round(med, 4), "min_ms": round(min(tot), 4), "max_ms": round(max(tot), 4),
                "phases_ms": {k: round(v, 4) for k, v in zip(PHASES, ph)}}

    def wide(self, v, reps, warmup, window_bits=0):
        self.e.h2d(self.d_sc, widen(v, self.s["fr_bytes"] // 8))
        return self.time(lambda: self.e.msm_device(self.curve, self.group, self.d_aff, self.d_sc, self.n, self.d_out,
                                                   scalars_plain=True, window_bits=window_bits), reps, warmup)

    def short(self, v, kind, reps, warmup, window_bits=0):
        self.e.h2d(self.d_sc, v)
        return self.time(lambda: self.e.msm_device_short(self.curve, self.group, self.d_aff, self.d_sc, kind, self.n,
                                                         self.d_out, window_bits=window_bits), reps, warmup)


def values(kind_name, n):
    _, dt = KINDS[kind_name]
    return np.random.default_rng(n).integers(0, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)


def emit(**row):
    print(json.dumps(row), flush=True)


def table_old_vs_new(args, only_wide=False):
    for gname, (curve, group) in GROUPS.items():
        for logn in (16, 20):
            b = Bench(curve, group, 1 << logn)
            for kname, (kind, _) in KINDS.items():
                v = values(kname, 1 << logn)
                emit(table="wide_fr", library=os.environ.get("AMDMSM_LIBRARY", "this"), group=gname, log2n=logn, values=kname,
                     **b.wide(v, args.reps, args.warmup))
                if not only_wide:
                    plan = b.la.plan_short(curve, group, 1 << logn, 8 * kind)
                    emit(table="short", group=gname, log2n=logn, values=kname, c=plan["c"], windows=plan["num_windows"],
                         **b.short(v, kind, args.reps, args.warmup))
            b.e.close()


def table_sweep(args):
    curve, group = GROUPS["alt_bn128_g1"]
    for logn in (16, 20):
        b = Bench(curve, group, 1 << logn)
        for kname, (kind, _) in KINDS.items():
            v = values(kname, 1 << logn)
            plan = b.la.plan_short(curve, group, 1 << logn, 8 * kind)
            emit(table="sweep", log2n=logn, bits=8 * kind, c="planner", chosen_c=plan["c"], **b.short(v, kind, args.reps, args.warmup))
            for c in range(6, 17):
                emit(table="sweep", log2n=logn, bits=8 * kind, c=c, **b.short(v, kind, args.reps, args.warmup, window_bits=c))
        b.e.close()


def table_host(args):
    import libff_amd

    curve, group = GROUPS["alt_bn128_g1"]
    n = 1 << 20
    e = libff_amd.Engine(0)
    s = libff_amd.sizes(curve, group)
    bases = e.gen_bases_seq(curve, group, n)
    h = e.register_bases(curve, group, bases, base_form=libff_amd.multi_exp_base_form_special)
    v = values("u32", n)
    w = widen(v, s["fr_bytes"] // 8)
    for name, call in (("wide_fr", lambda: e.multi_exp(curve, group, bases, w, base_form=1, scalars_plain=True)),
                       ("short_u32", lambda: e.multi_exp_short(curve, group, bases, v, base_form=1))):
        for _ in range(args.warmup):
            call()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        emit(table="host", route=name, log2n=20, scalar_bytes=int((w if name == "wide_fr" else v).nbytes),
             median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    e.unregister_bases(h)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--old", help="library of the parent commit: time its amdmsm_msm_device on the widened values")
    ap.add_argument("--only-wide", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if a.old:
        env = dict(os.environ, AMDMSM_LIBRARY=os.path.abspath(a.old))
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--only-wide", "--reps", str(a.reps), "--warmup",
                                  str(a.warmup)], env=env))
    if a.sweep:
        table_sweep(a)
    elif a.host:
        table_host(a)
    else:
        table_old_vs_new(a, only_wide=a.only_wide)
