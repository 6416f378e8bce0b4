#!/usr/bin/env python3
"""The four G1 MSMs of a Groth16 prover, two ways (bench.py stays the flagship's yardstick).

Shape: bases (i + 1) G of m + 1 points registered once; per proof one assignment of m + 1 scalars in host memory and the
m - 1 coefficients of H.  A runs over the whole assignment, L over the slice from l + 1 (l = 2^10), B over every second
position (a sorted index list), H over its own vector.

  (a) baseline   what a caller of the entries before amdmsm_multi_exp_batch_items does: B's scalars gathered on the
                 host with numpy, then four multi_exp calls (each uploads its scalars)
  (b) items      one multi_exp_batch_items call: the assignment uploaded once, slice and index list selected on the device

Host wall time per proof around calls that end in a synchronise, --reps proofs after --warmup, the two ways alternating.
(b) also reports the device phases of the batch (amdmsm_get_timings) and the bytes each way sends over PCIe, computed
from the shapes.  One JSON line per configuration.  --only baseline needs nothing newer than multi_exp, so it also
runs against a library built from an earlier commit (AMDMSM_LIBRARY=...).

  python tools/bench_batch_items.py [--configs alt_bn128_g1:20 alt_bn128_g1:22 bls12_377_g1:20] [--reps 20]

For k_sort_digits with and without an index list run it under rocprofv3 --kernel-trace --stats in a run of its own
(--only items): the trace lists k_sort_digits (H, own vector) and k_sort_digits_sel (A, L: slices; B: index list);
--index-as-slice replaces B's list by the slice of the same length, so the difference of two runs is the gather.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libff_amd  # noqa: E402

GROUPS = {"alt_bn128_g1": (libff_amd.ALT_BN128, libff_amd.G1), "bls12_377_g1": (libff_amd.BLS12_377, libff_amd.G1),
          "bls12_381_g1": (libff_amd.BLS12_381, libff_amd.G1), "mnt4_g1": (libff_amd.MNT4, libff_amd.G1)}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": round(float(np.median(a)), 3), "min": round(float(a[0]), 3), "max": round(float(a[-1]), 3),
            "p10": round(float(a[len(a) // 10]), 3), "p90": round(float(a[(9 * len(a)) // 10]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["alt_bn128_g1:20", "alt_bn128_g1:22", "bls12_377_g1:20"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "baseline", "items"], default="both")
    ap.add_argument("--index-as-slice", action="store_true")
    a = ap.parse_args()
    eng = libff_amd.Engine(0)
    rng = np.random.default_rng(1)
    special = libff_amd.multi_exp_base_form_special
    for cfg in a.configs:
        name, lg = cfg.split(":")
        curve, group = GROUPS[name]
        s = libff_amd.sizes(curve, group)
        m, l = 1 << int(lg), 1 << 10
        fl = s["fr_bytes"] // 8
        bases = eng.gen_bases_seq(curve, group, m + 1)
        handle = eng.register_bases(curve, group, bases, special)

        def scalars(n):
            sc = rng.integers(0, 1 << 63, size=(n, fl), dtype=np.uint64)
            sc[:, -1] &= np.uint64((1 << (s["fr_bits"] - 1 - 64 * (fl - 1))) - 1)   # below r: plain scalars
            return sc
        shared, own = scalars(m + 1), scalars(m - 1)
        idx = np.arange(0, m + 1, 2, dtype=np.uint32)
        nb = len(idx)

        def baseline():
            t0 = time.perf_counter()
            b_sc = shared[idx]   # the gather a caller does on the host today
            outs = [eng.multi_exp(curve, group, bases, shared, base_form=special, scalars_plain=True),
                    eng.multi_exp(curve, group, bases[l + 1:], shared[l + 1:], base_form=special, scalars_plain=True),
                    eng.multi_exp(curve, group, bases[:nb], b_sc, base_form=special, scalars_plain=True),
                    eng.multi_exp(curve, group, bases[:m - 1], own, base_form=special, scalars_plain=True)]
            return (time.perf_counter() - t0) * 1e3, outs

        def items():
            from libff_amd import BatchItem
            b_item = BatchItem(bases[:nb], offset=0) if a.index_as_slice else BatchItem(bases[:nb], index=idx)
            its = [BatchItem(bases), BatchItem(bases[l + 1:], offset=l + 1), b_item, BatchItem(bases[:m - 1], scalars=own)]
            t0 = time.perf_counter()
            outs = eng.multi_exp_batch_items(curve, group, its, shared, base_form=special, scalars_plain=True)
            return (time.perf_counter() - t0) * 1e3, outs

        ways = [w for w in (("baseline", baseline), ("items", items)) if a.only in ("both", w[0])]
        try:
            times = {w: [] for w, _ in ways}
            phases, results = [], {}
            eng.set_timing(True)
            for it in range(a.warmup + a.reps):
                for w, fn in ways:   # alternating
                    ms, outs = fn()
                    results[w] = outs
                    if it >= a.warmup:
                        times[w].append(ms)
                        if w == "items":
                            phases.append(eng.get_timings())
            eng.set_timing(False)
            fr = s["fr_bytes"]
            row = {"group": name, "log2m": int(lg), "reps": a.reps,
                   "pcie_scalar_bytes": {"baseline": fr * ((m + 1) + (m - l) + nb + (m - 1)),
                                         "items": fr * ((m + 1) + (m - 1)) + (0 if a.index_as_slice else 4 * nb)}}
            for w, _ in ways:
                row[w + "_ms"] = stats(times[w])
            if phases:
                tot = [p["total_ms"] for p in phases]
                med = phases[int(np.argsort(tot)[len(tot) // 2])]
                row["items_device_phases_ms_of_median"] = {k: round(v, 3) for k, v in med.items()}
            if len(ways) == 2:
                row["same_results"] = bool(all((x == y).all() for x, y in zip(results["baseline"], results["items"]))
                                           ) if not a.index_as_slice else None
            print(json.dumps(row), flush=True)
        finally:
            eng.unregister_bases(handle)


if __name__ == "__main__":
    main()
