#!/usr/bin/env python3
"""Time of the element-wise scalar multiplication on device-resident inputs (DESIGN section 13,
profiles/scalar_mul_vec.txt).

  python tools/scalar_mul_vec_time.py [10,16,20] [alt_bn128_g1 bls12_377_g2 mnt4_g1]

Per group and size, the median of 10 runs after 2 warm-ups of
  (a) amdmsm_scalar_mul_vec_device (OUT_AFFINE, automatic chunks), the call and the synchronise behind it;
  (b) at 2^10 only, the route there was before: a loop of amdmsm_msm_device with n = 1 over the resident points,
      one launch chain and one synchronise per element;
  (c) amdmsm_madd_bench_device at the same lane count with as many dependent mixed additions per lane as the ladder has
      group operations (w doublings and one addition per window of a w = 4 ladder over the scalar's words): the
      arithmetic ceiling, XYZZ additions with operands in registers.
and the share of (a) in table, ladder and normalisation, from the engine's phase timers (first chunk).
Points are (3 + i) G made on the device; scalars are random integers below 2^(fr_bits - 1), passed as plain integers."""
import ctypes
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


def median_ms(fn, runs=RUNS, warm=WARM):
    out = []
    for i in range(warm + runs):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    lgs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "10,16,20").split(",")]
    groups = sys.argv[2:] or ["alt_bn128_g1", "bls12_377_g2", "mnt4_g1"]
    eng = libff_amd.Engine(0)
    print("one run on one device; medians of %d after %d warm-ups" % (RUNS, WARM))
    for name in groups:
        cname, g = name.rsplit("_g", 1)
        curve, group = NAMES[cname], int(g)
        s = libff_amd.sizes(curve, group)
        fl = s["fr_bytes"] // 8
        for lg in lgs:
            n = 1 << lg
            sc = np.random.default_rng(lg).integers(0, 1 << 64, size=(n, fl), dtype=np.uint64)
            top = (s["fr_bits"] - 1) - 64 * (fl - 1)
            sc[:, fl - 1] &= np.uint64((1 << top) - 1) if top > 0 else np.uint64(0)
            d_aff, d_sc, d_out = eng.malloc(n * s["affine_bytes"]), eng.malloc(sc.nbytes), eng.malloc(n * s["g_bytes"])
            eng.gen_bases_seq_device(curve, group, 2, n, d_aff)
            eng.h2d(d_sc, sc)
            eng.synchronize()

            def vec():
                eng.scalar_mul_vec_device(curve, group, d_aff, d_sc, n, d_out, out_form=libff_amd.OUT_AFFINE, scalars_plain=True)
                eng.synchronize()

            a = median_ms(vec)
            eng.set_timing(True)
            vec()
            ph = eng.get_timings()
            eng.set_timing(False)
            table, ladder, norm = ph["scatter_ms"], ph["accumulate_ms"], ph["reduce_ms"]
            first = table + ladder + norm
            line = (f"{name} 2^{lg}: (a) vec {a:10.3f} ms = {a * 1e3 / n:9.3f} us/element; first chunk: table "
                    f"{100 * table / first:4.1f} % ladder {100 * ladder / first:4.1f} % normalise {100 * norm / first:4.1f} %")
            if lg == 10:
                d_one = eng.malloc(s["g_bytes"])

                def loop():
                    for i in range(n):
                        eng.msm_device(curve, group, ctypes.c_void_p(d_aff.value + i * s["affine_bytes"]),
                                       ctypes.c_void_p(d_sc.value + i * s["fr_bytes"]), 1, d_one, out_form=libff_amd.OUT_AFFINE,
                                       scalars_plain=True)
                        eng.synchronize()

                b = median_ms(loop)
                eng.free(d_one)
                line += f"; (b) loop of msm n=1 {b:10.3f} ms = {b * 1e3 / n:9.3f} us/element, (a)/(b) = {a / b:.4f}"
            iters = 5 * 8 * (s["fr_bytes"] // 4)
            ms = ctypes.c_float()

            def madd():
                eng._check(eng.lib.amdmsm_madd_bench_device(eng.h, curve, group, d_aff, d_out, ctypes.c_size_t(n), iters, 2,
                                                            ctypes.byref(ms)), "amdmsm_madd_bench_device")
                eng.synchronize()

            c = median_ms(madd)
            line += f"; (c) {iters} mixed additions per lane {c:10.3f} ms, (a)/(c) = {a / c:.2f}"
            print(line, flush=True)
            for p in (d_aff, d_sc, d_out):
                eng.free(p)


if __name__ == "__main__":
    main()
