#!/usr/bin/env python3
"""Device-resident MSM time of the MNT4-298 G1 / G2 and MNT6-298 G1 groups (bench.py stays the flagship's yardstick):
bases from gen_bases_seq and random scalars in HBM, amdmsm_msm_device timed per call by the engine's device events
(amdmsm_set_timing: total and phases), next to bls12_377 G1 / G2 -- the 12-word field, 253-bit
scalars -- as the comparison point.  One JSON line per (group, size).

  python tools/bench_mnt.py [--log2n 16 20 22] [--reps 10]

For the kernel statistics run it under rocprofv3 --kernel-trace --stats in a run of its own.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libff_amd  # noqa: E402

GROUPS = [("mnt4_g1", libff_amd.MNT4, libff_amd.G1), ("mnt4_g2", libff_amd.MNT4, libff_amd.G2),
          ("mnt6_g1", libff_amd.MNT6, libff_amd.G1), ("bls12_377_g1", libff_amd.BLS12_377, libff_amd.G1),
          ("bls12_377_g2", libff_amd.BLS12_377, libff_amd.G2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", default=",".join(g[0] for g in GROUPS))
    a = ap.parse_args()
    eng = libff_amd.Engine(0)
    rng = np.random.default_rng(1)
    for name, curve, group in GROUPS:
        if name not in a.groups.split(","):
            continue
        s = libff_amd.sizes(curve, group)
        for lg in a.log2n:
            n = 1 << lg
            d_b = eng.malloc(n * s["affine_bytes"])
            d_s = eng.malloc(n * s["fr_bytes"])
            d_o = eng.malloc(s["g_bytes"])
            try:
                eng.gen_bases_seq_device(curve, group, 0, n, d_b.value)
                sc = rng.integers(0, 1 << 63, size=(n, s["fr_bytes"] // 8), dtype=np.uint64)
                sc[:, -1] &= np.uint64((1 << (s["fr_bits"] - 1 - 64 * (s["fr_bytes"] // 8 - 1))) - 1)   # below r
                eng.h2d(d_s, sc)
                run = lambda: eng.msm_device(curve, group, d_b.value, d_s.value, n, d_o.value, scalars_plain=True)
                eng.set_timing(True)
                for _ in range(2):
                    run()
                phs = []
                for _ in range(a.reps):
                    run()
                    phs.append(eng.get_timings())   # device events of the call (waits for it)
                eng.set_timing(False)
                tot = [p["total_ms"] for p in phs]
                med = phs[int(np.argsort(tot)[len(tot) // 2])]
                plan = libff_amd.plan(curve, group, n)
                print(json.dumps({"group": name, "log2n": lg, "ms_median": round(float(np.median(tot)), 3),
                                  "ms_min": round(min(tot), 3), "c": plan["c"], "windows": plan["num_windows"],
                                  "phases_ms_of_median": {k: round(v, 3) for k, v in med.items()}}), flush=True)
            finally:
                for p in (d_b, d_s, d_o):
                    eng.free(p)


if __name__ == "__main__":
    main()
