#!/usr/bin/env python3
"""Time of the Lagrange vector of a domain on device-resident Montgomery records, against the batch inversion it ends in
and the powers call it is measured by, and the host time of the transposed matrix load (DESIGN section 24,
profiles/fr_lagrange.txt).

  python tools/fr_lagrange_time.py [--out profiles/fr_lagrange.txt] [alt_bn128:20,20+19,20+10,20+0 bls12_377:...]
  python tools/fr_lagrange_time.py --transpose [rows_log2 entries_log2]      the load alone, default 20 22

Per curve and m = 2^b or 2^b + 2^s, medians of 10 runs after 2 warm-ups, one process:
  the call and the synchronise behind it of amdmsm_fr_domain_lagrange_device, of amdmsm_fr_batch_invert_device at n = m
  and of amdmsm_fr_powers_device at n = m (the wall time of the last: it has no phases of its own);
  the kernels phase of the first two from the engine's timers (a run of their own), and from them
      sweep = kernels(lagrange) - kernels(batch_invert, n = m):   k_frd_lagrange alone
The sweep writes m records once and reads one power of w per record; so does k_fr_powers, with one product per record
in its loop and log2(lanes) more per lane before it -- at 2^20 records on 2^16 lanes 16 + 16 products for 16 records, two
per record -- where the sweep has two (and one more load below B of a step domain).  Both times and their ratio are
reported, with the spread of the two kernels phases, whose difference the sweep is; a ratio above 2 is to be explained
from tools/kernel_resources.py, not tuned away."""
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
DEFAULT = ["alt_bn128:20,20+19,20+10,20+0", "bls12_377:20,20+19,20+10,20+0"]


def random_records(curve, n, seed):
    """n canonical records: any value below 2^(bits - 1) is one"""
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    return a


def measure(eng, fn, phases=True):
    """(median wall ms, min, max, median kernels-phase ms, its min, its max) of fn, which enqueues one call"""
    def once():
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    wall = [once() for _ in range(WARM + RUNS)][WARM:]
    kern = [0.0]
    if phases:
        eng.set_timing(True)
        try:
            kern = []
            for _ in range(RUNS):
                fn()
                kern.append(eng.get_timings()["scatter_ms"])
        finally:
            eng.set_timing(False)
    return statistics.median(wall), min(wall), max(wall), statistics.median(kern), min(kern), max(kern)


def transpose_times(eng, emit, rows_log2, entries_log2):
    """host time of amdmsm_fr_matrix_load and of amdmsm_fr_matrix_load_transposed on one random matrix, one load each
    after one warm-up: a one-off per key, no bar"""
    curve = 0
    n_rows, nnz = 1 << rows_log2, 1 << entries_log2
    rng = np.random.default_rng(7)
    per = nnz // n_rows
    offsets = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(per)
    cols = rng.integers(0, n_rows, size=nnz, dtype=np.uint32)
    cols[::per] = 0   # the column of the constant 1 in every row
    coeffs = random_records(curve, nnz, 8)
    for name, load in (("load", eng.fr_matrix_load), ("load_transposed", eng.fr_matrix_load_transposed)):
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            mat = load(curve, offsets, cols, coeffs, n_rows)
            times.append((time.perf_counter() - t0) * 1e3)
            mat.free()
        emit(f"alt_bn128 2^{rows_log2} rows, 2^{entries_log2} entries, column 0 in every row: fr_matrix_{name} {times[1]:.1f} ms "
             f"(first call {times[0]:.1f} ms)")


def main():
    args = sys.argv[1:]
    out = None
    if args[:1] == ["--out"]:
        out, args = open(args[1], "a"), args[2:]

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    eng = libff_amd.Engine(0)
    if args[:1] == ["--transpose"]:
        lg = [int(x) for x in args[1:3]] or [20, 22]
        return transpose_times(eng, emit, *lg)
    emit("one run on one device; medians of %d after %d warm-ups; one process; Montgomery records" % (RUNS, WARM))
    for spec in args or DEFAULT:
        cname, shapes = spec.split(":")
        curve = NAMES[cname]
        r = libff_amd.fr_modulus(curve, libff_amd.G1)
        rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
        for shape in shapes.split(","):
            parts = [int(x) for x in shape.split("+")]
            m = sum(1 << p for p in parts)
            assert libff_amd.fr_domain(curve, m)["m"] == m, shape
            t = int.from_bytes(np.random.default_rng(m).bytes(rec), "little") % r
            recs = random_records(curve, m, m & 0xffff)
            d_in, d_out = eng.malloc(recs.nbytes), eng.malloc(recs.nbytes)
            eng.h2d(d_in, recs)
            lag = measure(eng, lambda: eng.fr_domain_lagrange_device(curve, m, t, d_out))
            inv = measure(eng, lambda: eng.fr_batch_invert_device(curve, m, d_in, d_out))
            pw = measure(eng, lambda: eng.fr_powers_device(curve, t, m, d_out), phases=False)
            sweep = lag[3] - inv[3]
            name = " + ".join(f"2^{p}" for p in parts)
            emit(f"{cname} m = {name}: lagrange {lag[0]:.4f} ms [min {lag[1]:.4f} max {lag[2]:.4f}], kernels {lag[3]:.4f} ms "
                 f"[min {lag[4]:.4f} max {lag[5]:.4f}]; batch_invert n = m {inv[0]:.4f} ms, kernels {inv[3]:.4f} ms "
                 f"[min {inv[4]:.4f} max {inv[5]:.4f}]; powers n = m {pw[0]:.4f} ms [min {pw[1]:.4f} max {pw[2]:.4f}]")
            emit(f"  sweep = {sweep:.4f} ms = {sweep / pw[0]:.2f} of the powers call, {m * rec / max(sweep, 1e-9) / 1e6:.0f} GB/s written"
                 f"{'' if sweep <= 2 * pw[0] else ': ABOVE TWICE the powers call'}")
            eng.free(d_in)
            eng.free(d_out)
    transpose_times(eng, emit, 20, 22)
    if out:
        out.close()


if __name__ == "__main__":
    main()
