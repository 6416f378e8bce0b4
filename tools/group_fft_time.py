#!/usr/bin/env python3
"""Time of the radix-2 FFT over a point vector on device-resident inputs (profiles/group_fft.txt).

  python tools/group_fft_time.py [alt_bn128_g1:10,16,20 bls12_377_g2:10,16,20 mnt4_g1:16]

Per group and size n = 2^lg, the median of 10 runs after 2 warm-ups of
  (a) amdmsm_group_fft_device (OUT_AFFINE, automatic chunks), the call and the synchronise behind it;
  (b) the same ladders, tables and normalisations on half the records: (lg - 1) calls of amdmsm_scalar_mul_vec_device on
      n / 2 elements with OUT_AFFINE, synchronised once.  That entry and its kernels are the parent commit's, unchanged
      (tools/asm_identity.py), so it runs from this library in this process.  The runs of (a) and (b) alternate;
and the phases of (a) summed over its stages, from the engine's timers in a run of their own.
The points are 3 G, 4 G, ... made on the device; the twiddles are the plain powers of fft_twiddles; the scalars of (b) are
the same powers, each twice."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libff_amd  # noqa: E402

NAMES = {"alt_bn128": 0, "bls12_377": 1, "bw6_761": 2, "bls12_381": 3, "mnt4": 4, "mnt6": 5}
RUNS, WARM = 10, 2
DEFAULT = ["alt_bn128_g1:10,16,20", "bls12_377_g2:10,16,20", "mnt4_g1:16"]


def ids(name):
    cname, g = name.rsplit("_g", 1)
    return NAMES[cname], int(g)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    eng = libff_amd.Engine(0)
    print("one run on one device; medians of %d after %d warm-ups; (a) and (b) alternate" % (RUNS, WARM))
    for spec in sys.argv[1:] or DEFAULT:
        name, lgs = spec.split(":")
        curve, group = ids(name)
        s = libff_amd.sizes(curve, group)
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            tw = libff_amd.fft_twiddles(curve, n)
            d_aff, d_out = eng.malloc(n * s["affine_bytes"]), eng.malloc(n * s["g_bytes"])
            d_tw = eng.malloc(tw.nbytes)
            eng.gen_bases_seq_device(curve, group, 2, n, d_aff)
            eng.h2d(d_tw, tw)
            eng.synchronize()
            p = libff_amd.plan_group_fft(curve, group, n)

            def fft():
                eng.group_fft_device(curve, group, d_aff, n, d_tw, d_out, out_form=libff_amd.OUT_AFFINE, scalars_plain=True)
                eng.synchronize()

            def smv():
                for _ in range(lg - 1):
                    eng.scalar_mul_vec_device(curve, group, d_aff, d_tw, n // 2, d_out, out_form=libff_amd.OUT_AFFINE,
                                              scalars_plain=True)
                eng.synchronize()

            a, b = [], []
            for i in range(WARM + RUNS):
                ta, tb = timed(fft), timed(smv)
                if i >= WARM:
                    a.append(ta)
                    b.append(tb)
            ma, mb = statistics.median(a), statistics.median(b)
            eng.set_timing(True)
            fft()
            ph = eng.get_timings()
            eng.set_timing(False)
            parts = [ph["count_ms"], ph["scatter_ms"], ph["accumulate_ms"], ph["reduce_ms"]]
            tot = max(ph["total_ms"], 1e-9)
            print(f"{name} 2^{lg}: {p['stages']} stages, {p['scalar_muls']} scalar multiplications, chunks of {p['chunk_points']} "
                  f"butterflies, workspace {p['workspace_bytes'] / 2 ** 20:.1f} MiB; "
                  f"(a) {ma:10.3f} ms [min {min(a):.3f} max {max(a):.3f}] = {ma * 1e6 / max(p['scalar_muls'], 1):7.2f} ns per scalar multiplication; "
                  f"(b) {lg - 1} x scalar_mul_vec on n/2 {mb:10.3f} ms [min {min(b):.3f} max {max(b):.3f}]; (a)/(b) = {ma / mb:.3f}; "
                  f"phases of a timed (a), {ph['total_ms']:.3f} ms: import {100 * parts[0] / tot:4.1f} % gathers and tables "
                  f"{100 * parts[1] / tot:4.1f} % ladders and butterflies {100 * parts[2] / tot:4.1f} % normalisations and export "
                  f"{100 * parts[3] / tot:4.1f} %", flush=True)
            for d in (d_aff, d_out, d_tw):
                eng.free(d)


if __name__ == "__main__":
    main()
