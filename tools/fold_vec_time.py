#!/usr/bin/env python3
"""Time of the fold of point vectors on device-resident inputs (profiles/fold_vec.txt).

  python tools/fold_vec_time.py [16,20] [1,2,8] [alt_bn128_g1 bls12_377_g2 mnt4_g1] [--baseline PATH/libamdmsm.so]

Per group, size n and number of vectors k, the median of 10 runs after 2 warm-ups of
  (a) amdmsm_fold_vec_device (OUT_LIBFF, automatic chunks) without the endomorphism split, the call and the synchronise
      behind it, and where the group permits it (a+) the same with the split;
  (b) with --baseline, the only route there was before, through the library given (a build of the parent commit, loaded
      by a worker process of this script through AMDMSM_LIBRARY): k calls of amdmsm_scalar_mul_vec_device with each scalar
      replicated n times, synchronised once.  The k - 1 vector additions that route would still owe are left out, which
      favours it.  The runs of (a), (a+) and (b) alternate, one of each per round;
  (c) amdmsm_madd_bench_device at the same lane count with as many dependent mixed additions per lane as the ladder of (a)
      / (a+) has group operations (4 doublings per window and 15/16 of an addition per row and window): the arithmetic
      ceiling, XYZZ additions with operands in registers;
and the share of (a) / (a+) in digits and tables, ladder and export, from the engine's phase timers (first chunk).
Vector j is ((2 + j n) + i + 1) G made on the device; the scalars are random integers below 2^(fr_bits - 1), passed as
plain integers."""
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
import libff_amd  # noqa: E402

NAMES = {"alt_bn128": 0, "bls12_377": 1, "bw6_761": 2, "bls12_381": 3, "mnt4": 4, "mnt6": 5}
RUNS, WARM = 10, 2


def ids(name):
    cname, g = name.rsplit("_g", 1)
    return NAMES[cname], int(g)


def scalars(curve, group, k, seed):
    s = libff_amd.sizes(curve, group)
    fl = s["fr_bytes"] // 8
    sc = np.random.default_rng(seed).integers(0, 1 << 64, size=(k, fl), dtype=np.uint64)
    top = (s["fr_bits"] - 1) - 64 * (fl - 1)
    sc[:, fl - 1] &= np.uint64((1 << top) - 1) if top > 0 else np.uint64(0)
    return sc


class Vectors:
    """k resident vectors of n points and an output vector"""

    def __init__(self, eng, curve, group, k, n):
        s = libff_amd.sizes(curve, group)
        self.eng = eng
        self.d_vecs = [eng.malloc(n * s["affine_bytes"]) for _ in range(k)]
        self.d_out = eng.malloc(n * s["g_bytes"])
        for j, d in enumerate(self.d_vecs):
            eng.gen_bases_seq_device(curve, group, 2 + j * n, n, d)
        eng.synchronize()

    def free(self):
        for p in self.d_vecs + [self.d_out]:
            self.eng.free(p)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def baseline_worker():
    """the route before the fold, in a process of its own that has loaded the library AMDMSM_LIBRARY names: one JSON
    request per line on stdin, one reply per line on stdout"""
    eng = libff_amd.Engine(0)
    state = {}
    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "setup":
            curve, group, k, n = req["curve"], req["group"], req["k"], req["n"]
            v = Vectors(eng, curve, group, k, n)
            sc = scalars(curve, group, k, req["seed"])
            d_sc = []
            for j in range(k):
                d = eng.malloc(n * sc.shape[1] * 8)
                eng.h2d(d, np.repeat(sc[j:j + 1], n, axis=0))
                d_sc.append(d)
            eng.synchronize()
            state = {"v": v, "d_sc": d_sc, "args": (curve, group, k, n)}
            reply = {"ok": True}
        elif req["op"] == "run":
            curve, group, k, n = state["args"]

            def route():
                for j in range(k):
                    eng.scalar_mul_vec_device(curve, group, state["v"].d_vecs[j], state["d_sc"][j], n, state["v"].d_out,
                                              out_form=libff_amd.OUT_LIBFF, scalars_plain=True)
                eng.synchronize()

            reply = {"ms": timed(route)}
        elif req["op"] == "teardown":
            state["v"].free()
            for d in state["d_sc"]:
                eng.free(d)
            state = {}
            reply = {"ok": True}
        else:
            break
        print(json.dumps(reply), flush=True)


class Baseline:
    def __init__(self, library):
        env = dict(os.environ, AMDMSM_LIBRARY=os.path.abspath(library))
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--baseline-worker"], env=env, text=True,
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def ask(self, **req):
        self.p.stdin.write(json.dumps(req) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the baseline worker has ended (exit code %s)" % self.p.poll())
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def main():
    args = sys.argv[1:]
    if args == ["--baseline-worker"]:
        return baseline_worker()
    library = None
    if "--baseline" in args:
        i = args.index("--baseline")
        library = args[i + 1]
        del args[i:i + 2]
    lgs = [int(x) for x in (args[0] if args else "16,20").split(",")]
    ks = [int(x) for x in (args[1] if len(args) > 1 else "1,2,8").split(",")]
    groups = args[2:] or ["alt_bn128_g1", "bls12_377_g2", "mnt4_g1"]
    base = Baseline(library) if library else None   # started before this process opens the device
    eng = libff_amd.Engine(0)
    print("one run on one device; medians of %d after %d warm-ups; (a) / (a+) / (b) alternate" % (RUNS, WARM))
    try:
        for name in groups:
            curve, group = ids(name)
            modes = [(-1, "(a) ")] + ([(2, "(a+)")] if libff_amd.plan_fold(curve, group, 1, 1, endomorphism=2)["endomorphism"] else [])
            for lg in lgs:
                n = 1 << lg
                for k in ks:
                    v = Vectors(eng, curve, group, k, n)
                    sc = scalars(curve, group, k, lg * 16 + k)
                    if base:
                        base.ask(op="setup", curve=curve, group=group, k=k, n=n, seed=lg * 16 + k)

                    def fold(value):
                        eng.endomorphism = value
                        eng.fold_vec_device(curve, group, v.d_vecs, sc, n, v.d_out, out_form=libff_amd.OUT_LIBFF, scalars_plain=True)
                        eng.synchronize()

                    times = {value: [] for value, _ in modes}
                    times["base"] = []
                    for i in range(WARM + RUNS):
                        for value, _ in modes:
                            t = timed(lambda: fold(value))
                            if i >= WARM:
                                times[value].append(t)
                        if base:
                            t = base.ask(op="run")["ms"]
                            if i >= WARM:
                                times["base"].append(t)
                    b = statistics.median(times["base"]) if base else None
                    for value, tag in modes:
                        a = statistics.median(times[value])
                        p = libff_amd.plan_fold(curve, group, k, n, endomorphism=value)
                        eng.set_timing(True)
                        fold(value)
                        ph = eng.get_timings()
                        eng.set_timing(False)
                        tables, ladder, export = ph["scatter_ms"], ph["accumulate_ms"], ph["reduce_ms"]
                        first = max(tables + ladder + export, 1e-9)
                        iters = int(round(p["num_windows"] * (4 + p["rows"] * 15 / 16)))
                        ms = ctypes.c_float()

                        def madd():
                            eng._check(eng.lib.amdmsm_madd_bench_device(eng.h, curve, group, v.d_vecs[0], v.d_out, ctypes.c_size_t(n),
                                                                        iters, 2, ctypes.byref(ms)), "amdmsm_madd_bench_device")
                            eng.synchronize()

                        c = statistics.median([timed(madd) for _ in range(1 + 5)][1:])
                        line = (f"{name} 2^{lg} k={k} {tag} {p['rows']:2d} rows x {p['num_windows']:2d} windows, chunks of {p['chunk_points']}: "
                                f"{a:10.3f} ms = {a * 1e3 / n:8.3f} us/element; first chunk: tables {100 * tables / first:4.1f} % "
                                f"ladder {100 * ladder / first:4.1f} % export {100 * export / first:4.1f} %")
                        if base:
                            line += f"; (b) {k} x scalar_mul_vec {b:10.3f} ms, {tag.strip()}/(b) = {a / b:.3f}"
                        line += f"; (c) {iters} mixed additions per lane {c:10.3f} ms, {tag.strip()}/(c) = {a / c:.2f}"
                        print(line, flush=True)
                    if base:
                        base.ask(op="teardown")
                    v.free()
    finally:
        if base:
            base.close()


if __name__ == "__main__":
    main()
