#!/usr/bin/env python3
"""Time of the radix-2 FFT over Fr scalars on device-resident vectors, against the MSM it feeds (DESIGN section 18,
profiles/fr_fft.txt).

  python tools/fr_fft_time.py [--out profiles/fr_fft.txt] [alt_bn128:16,20,24 bls12_377:16,20,24 bw6_761:16,20,24]
  python tools/fr_fft_time.py --probe alt_bn128 20 [reps]     transforms only, for a counters run of its own:
      rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -- python tools/fr_fft_time.py --probe ...
  python tools/fr_fft_time.py --counters DIR                  sums those counters per kernel from rocprofv3's csv

Per curve and size n = 2^lg, the median of 10 runs after 2 warm-ups of
  (a) amdmsm_fr_fft_device, out of place, Montgomery records, the twiddles resident: the call and the synchronise behind it;
  (b) amdmsm_msm_device of the curve's G1 at the same n on the same scalars -- code this change leaves as the parent has
      it (tools/asm_identity.py) -- in the same process, the runs of (a) and (b) alternating;
  (c) the transform with the powers of omega rebuilt (three roots in turn over a cache of two), median of 5;
and the phases of (a) from the engine's timers in a run of their own.  Effective bytes: every pass reads and writes the
vector once.  Products: n / 2 * log2 n, one per butterfly.  The bar: (a) <= (b) / 4 at 2^20 for alt_bn128 and bls12_377."""
import csv
import glob
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
DEFAULT = ["alt_bn128:16,20,24", "bls12_377:16,20,24", "bw6_761:16,20,24"]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def random_records(curve, n, seed):
    """n canonical Montgomery records: any value below 2^(bits - 1) is one"""
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    return a


def probe(cname, lg, reps):
    curve, n = NAMES[cname], 1 << lg
    eng = libff_amd.Engine(0)
    recs = random_records(curve, n, 1)
    d_in, d_out = eng.malloc(recs.nbytes), eng.malloc(recs.nbytes)
    eng.h2d(d_in, recs)
    for _ in range(reps):
        eng.fr_fft_device(curve, d_in, n, d_out)
    eng.synchronize()
    print("done")


def counters(directory, emit=print):
    """per kernel and counter: dispatches and the sum over them, from the csv of a rocprofv3 --pmc run"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            key = (row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0], row["Counter_Name"])
            c = rows.setdefault(key, [0, 0.0])
            c[0] += 1
            c[1] += float(row["Counter_Value"])
    for (kernel, counter), (k, v) in sorted(rows.items()):
        emit(f"counters: {kernel} {counter}: {k} dispatches, sum {v:.0f}")
    return rows


def main():
    args = sys.argv[1:]
    if args[:1] == ["--probe"]:
        return probe(args[1], int(args[2]), int(args[3]) if len(args) > 3 else 3)
    if args[:1] == ["--counters"]:
        return counters(args[1])
    out = None
    if args[:1] == ["--out"]:
        out, args = open(args[1], "w"), args[2:]

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    eng = libff_amd.Engine(0)
    emit("one run on one device; medians of %d after %d warm-ups; (a) and (b) alternate in one process" % (RUNS, WARM))
    bar = {}
    for spec in args or DEFAULT:
        cname, lgs = spec.split(":")
        curve = NAMES[cname]
        s = libff_amd.sizes(curve, libff_amd.G1)
        r = libff_amd.fr_modulus(curve, libff_amd.G1)
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            try:
                w = libff_amd.fr_root_of_unity(curve, n)
            except ValueError:
                emit(f"{cname} 2^{lg}: above the field's 2-adicity, left out")
                continue
            recs = random_records(curve, n, lg)
            d_in, d_out = eng.malloc(recs.nbytes), eng.malloc(recs.nbytes)
            d_aff, d_res = eng.malloc(n * s["affine_bytes"]), eng.malloc(s["g_bytes"])
            eng.h2d(d_in, recs)
            eng.gen_bases_seq_device(curve, libff_amd.G1, 2, n, d_aff)
            eng.synchronize()
            p = libff_amd.plan_fr_fft(curve, n)

            def fft(omega=None):
                eng.fr_fft_device(curve, d_in, n, d_out, omega=omega)
                eng.synchronize()

            def msm():
                eng.msm_device(curve, libff_amd.G1, d_aff, d_in, n, d_res)
                eng.synchronize()

            a, b = [], []
            for i in range(WARM + RUNS):
                ta, tb = timed(fft), timed(msm)
                if i >= WARM:
                    a.append(ta)
                    b.append(tb)
            ma, mb = statistics.median(a), statistics.median(b)
            cold = statistics.median([timed(lambda: fft(pow(w, 2 * (i % 3) + 1, r))) for i in range(6)][1:])
            eng.set_timing(True)
            fft()
            ph = eng.get_timings()
            eng.set_timing(False)
            traffic = 2.0 * p["passes"] * n * s["fr_bytes"]
            emit(f"{cname} 2^{lg}: tile 2^{p['tile_log2']}, {p['passes']} passes, {p['butterflies']} butterflies, workspace "
                 f"{p['workspace_bytes'] / 2 ** 20:.1f} MiB; (a) fr_fft_device {ma:9.4f} ms [min {min(a):.4f} max {max(a):.4f}] = "
                 f"{traffic / ma / 1e6:7.1f} GB/s effective, {p['butterflies'] / ma / 1e6:7.2f} G products/s; (b) msm_device G1 "
                 f"{mb:9.4f} ms [min {min(b):.4f} max {max(b):.4f}]; (a)/(b) = {ma / mb:.4f}; (c) twiddles rebuilt {cold:9.4f} ms; "
                 f"phases of a timed (a), {ph['total_ms']:.4f} ms: twiddles and powers {ph['count_ms']:.4f} passes "
                 f"{ph['scatter_ms']:.4f} download {ph['accumulate_ms']:.4f}")
            if lg == 20 and cname in ("alt_bn128", "bls12_377"):
                bar[cname] = ma / mb
            for d in (d_in, d_out, d_aff, d_res):
                eng.free(d)
    for cname, ratio in bar.items():
        emit(f"bar, {cname} 2^20: one transform is {ratio:.4f} of the MSM it feeds (at most 0.25): "
             f"{'met' if ratio <= 0.25 else 'MISSED'}; seven transforms cost {7 * ratio:.2f} MSMs")
    if out:
        out.close()


if __name__ == "__main__":
    main()
