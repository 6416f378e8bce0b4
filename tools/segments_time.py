"""Time of the segmented MSM (amdmsm_msm_device_segments) against what a caller had before it, on device-resident inputs.

    python tools/segments_time.py                 # every table below
    python tools/segments_time.py --groups alt_bn128_g1 --tables routes

  routes   m segments of L terms, (m, L) = (2^10, 16), (2^10, 256), (2^14, 16):
             a        one amdmsm_msm_device_segments call, no segment on the single-MSM route (long_from = SIZE_MAX)
             b_loop   amdmsm_msm_device per segment, synchronised per call as a caller would have it      (m = 2^10 only)
             b_batch  amdmsm_msm_device_batch in groups of 8, synchronised per call                        (m = 2^10 only)
             c        amdmsm_scalar_mul_vec_device over all terms (engine-Jacobian records), then one
                      amdmsm_sum_points_device per segment, synchronised once
           with the phase times of (a): table / digits / accumulate / Horner / normalise and later chunks
  sweep    one segment of 2^8 .. 2^14 terms through both routes of the new entry (long_from = SIZE_MAX against 1): the
           crossover is the default long_from of the group's field width

Wall-clock milliseconds around one run that ends in a synchronise; median of --reps runs after --warmup (10 and 2).  A
route whose single run takes more than --slow-ms is timed with 3 runs after 1; its row says so ("reps").
Raw output: profiles/segmented_msm.txt.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"alt_bn128_g1": (0, 1), "bls12_377_g2": (1, 2), "mnt4_g1": (4, 1), "bw6_761_g1": (2, 1)}
SHAPES = [(1 << 10, 16), (1 << 10, 256), (1 << 14, 16)]
SIZE_MAX = 2 ** 64 - 1
PHASES = ("table", "digits", "accumulate", "horner", "normalise_and_rest", "total")


def emit(**row):
    print(json.dumps(row), flush=True)


class Bench:
    def __init__(self, curve, group, n_terms, m):
        import libff_amd

        self.la, self.e = libff_amd, libff_amd.Engine(0)
        self.curve, self.group, self.n = curve, group, n_terms
        self.s = s = libff_amd.sizes(curve, group)
        e = self.e
        self.d_aff, self.d_sc = e.malloc(n_terms * s["affine_bytes"]), e.malloc(n_terms * s["fr_bytes"])
        self.d_out, self.d_prod = e.malloc(max(m, 1) * s["g_bytes"]), e.malloc(n_terms * s["g_bytes"])
        e.gen_bases_seq_device(curve, group, 0, n_terms, self.d_aff)
        # plain integers below 2^(fr_bits - 1): below r for every group
        fl, rng = s["fr_bytes"] // 8, np.random.default_rng(n_terms)
        sc = rng.integers(0, 2 ** 63, size=(n_terms, fl), dtype=np.uint64, endpoint=False) * 2 + 1
        top, bits = (s["fr_bits"] - 1) // 64, (s["fr_bits"] - 1) % 64
        sc[:, top] &= np.uint64((1 << bits) - 1)
        sc[:, top + 1:] = 0
        e.h2d(self.d_sc, sc)
        e.synchronize()

    def close(self):
        for p in (self.d_aff, self.d_sc, self.d_out, self.d_prod):
            self.e.free(p)
        self.e.close()

    def time(self, run, args):
        def once():
            t0 = time.perf_counter()
            run()
            self.e.synchronize()
            return (time.perf_counter() - t0) * 1e3

        first = once()
        reps, warm = (3, 1) if first > args.slow_ms else (args.reps, args.warmup)
        for _ in range(max(warm - 1, 0)):
            once()
        t = [once() for _ in range(reps)]
        return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "reps": reps}

    def at(self, base, i, size):
        return ctypes.c_void_p(base.value + i * size)

    # ---- the routes
    def a(self, offs, long_from=SIZE_MAX):
        self.e.msm_device_segments(self.curve, self.group, self.d_aff, self.n, self.d_sc, self.n, offs, self.d_out,
                                   long_from=long_from, scalars_plain=True)

    def b_loop(self, offs):
        s, e = self.s, self.e
        for j in range(len(offs) - 1):
            lo, ln = int(offs[j]), int(offs[j + 1] - offs[j])
            e.msm_device(self.curve, self.group, self.at(self.d_aff, lo, s["affine_bytes"]), self.at(self.d_sc, lo, s["fr_bytes"]),
                         ln, self.at(self.d_out, j, s["g_bytes"]), scalars_plain=True)
            e.synchronize()

    def b_batch(self, offs, length):
        s, e = self.s, self.e
        for j0 in range(0, len(offs) - 1, 8):
            js = range(j0, min(j0 + 8, len(offs) - 1))
            e.msm_device_batch(self.curve, self.group, [self.at(self.d_aff, int(offs[j]), s["affine_bytes"]) for j in js],
                               [self.at(self.d_sc, int(offs[j]), s["fr_bytes"]) for j in js], length,
                               [self.at(self.d_out, j, s["g_bytes"]) for j in js], scalars_plain=True)
            e.synchronize()

    def c(self, offs):
        s, e = self.s, self.e
        e.scalar_mul_vec_device(self.curve, self.group, self.d_aff, self.d_sc, self.n, self.d_prod, out_form=self.la.OUT_JACOBIAN,
                                scalars_plain=True)
        for j in range(len(offs) - 1):
            lo, ln = int(offs[j]), int(offs[j + 1] - offs[j])
            e.sum_points_device(self.curve, self.group, self.at(self.d_prod, lo, s["g_bytes"]), ln, self.la.OUT_LIBFF,
                                self.at(self.d_out, j, s["g_bytes"]))


def table_routes(name, curve, group, args):
    for m, length in SHAPES:
        b = Bench(curve, group, m * length, m)
        offs = (np.arange(m + 1) * length).astype(np.uint64)
        row = dict(table="routes", group=name, segments=m, terms=length)
        ra = b.time(lambda: b.a(offs), args)
        b.e.set_timing(True)
        b.a(offs)
        ms = list(b.e.get_timings().values())   # the six phase slots in order
        b.e.set_timing(False)
        emit(route="a", **row, **ra, phases_ms={k: round(v, 4) for k, v in zip(PHASES, ms[:6])})
        results = {"a": ra}
        if m <= 1 << 10:
            results["b_loop"] = b.time(lambda: b.b_loop(offs), args)
            emit(route="b_loop", **row, **results["b_loop"])
            results["b_batch"] = b.time(lambda: b.b_batch(offs, length), args)
            emit(route="b_batch", **row, **results["b_batch"])
        results["c"] = b.time(lambda: b.c(offs), args)
        emit(route="c", **row, **results["c"])
        emit(table="ratios", group=name, segments=m, terms=length,
             **{f"{k}_over_a": round(v["median_ms"] / ra["median_ms"], 2) for k, v in results.items() if k != "a"})
        b.close()


def table_sweep(name, curve, group, args):
    cross = None
    for lg in range(8, 15):
        n = 1 << lg
        b = Bench(curve, group, n, 1)
        offs = np.array([0, n], dtype=np.uint64)
        seg = b.time(lambda: b.a(offs, SIZE_MAX), args)
        msm = b.time(lambda: b.a(offs, 1), args)
        if cross is None and msm["median_ms"] < seg["median_ms"]:
            cross = n
        emit(table="sweep", group=name, coordinate_bytes=b.s["affine_bytes"] // 2, log2_terms=lg,
             segment_route_ms=seg["median_ms"], single_msm_route_ms=msm["median_ms"])
        b.close()
    emit(table="long_from", group=name, first_size_where_the_single_msm_route_wins=cross)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-ms", type=float, default=1500.0)
    ap.add_argument("--groups", default="alt_bn128_g1,bls12_377_g2,mnt4_g1")
    ap.add_argument("--tables", default="routes,sweep")
    a = ap.parse_args()
    for gname in a.groups.split(","):
        cv, gr = GROUPS[gname]
        if "routes" in a.tables:
            table_routes(gname, cv, gr, a)
        if "sweep" in a.tables:
            table_sweep(gname, cv, gr, a)
