#!/usr/bin/env python3
"""Time of the sparse matrix times Fr vector on device-resident vectors, against the seven transforms it feeds and the
G1 MSM of the same size (profiles/fr_matrix.txt).

  python tools/fr_matrix_time.py [--out profiles/fr_matrix.txt] [--sweep] [alt_bn128:16,20,24 bls12_377:20 ...]
  python tools/fr_matrix_time.py --probe alt_bn128 20 [reps]     applies only, for a kernel trace or a counters run of its own

The workload is synthetic: a seeded matrix of the shape the issue behind this entry ASSUMES for R1CS -- no survey of
real circuits stands behind it.  Row lengths: 1 to 3 for nine rows in ten, 4 to 8 for most of the rest, 254 for one row
in a hundred, and one row of 2^16 (2^12 below 2^20 rows).  Coefficients: 1 for eight in ten, r - 1 for one in ten, the
rest powers of two and random values half and half.  Columns uniform over n_cols = n_rows.

Per curve and size n = 2^lg, medians of 10 runs after 2 warm-ups, Montgomery records resident on the device, each run the
calls and the synchronise behind them, (a) .. (d) alternating in one process:
  (a) three amdmsm_fr_matrix_apply_device of three such matrices (at 2^24: one matrix three times) on one vector;
  (b) the same with the handles loaded under AMDMSM_FR_MATRIX_NAIVE=1;
  (c) the seven amdmsm_fr_fft_device of the quotient recipe at n (three inverse, three coset, one inverse coset);
  (d) amdmsm_msm_device of the curve's G1 at n.
Effective bytes of an apply: per kept entry its 4-byte word and the record of x it reads, per general entry its
coefficient record too, per output record one store.  --sweep: (a) for one matrix under other row-class thresholds.
The extremes: one matrix with every coefficient general, one with every coefficient 1 or r - 1.
The target: (a) <= (c) for alt_bn128 at 2^20."""
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
DEFAULT = ["alt_bn128:16,20,24", "bls12_377:20", "bls12_381:20", "bw6_761:20"]
ENV_NAIVE, ENV_WAVE, ENV_SPLIT = "AMDMSM_FR_MATRIX_NAIVE", "AMDMSM_FR_MATRIX_WAVE_ROW", "AMDMSM_FR_MATRIX_SPLIT_ROW"


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def limbs_of(v, limbs):
    return np.frombuffer(int(v).to_bytes(8 * limbs, "little"), dtype="<u8").astype(np.uint64)


def synthetic(curve, lg, seed, mix="r1cs"):
    """(offsets, cols, plain coefficient records) of the assumed R1CS shape; mix: r1cs, general or unit"""
    n = 1 << lg
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    rng = np.random.default_rng(1000 * curve + 10 * lg + seed)
    kind = rng.random(n)
    lens = np.where(kind < 0.90, rng.integers(1, 4, n), np.where(kind < 0.99, rng.integers(4, 9, n), 254)).astype(np.uint64)
    lens[int(rng.integers(0, n))] = 1 << (16 if lg >= 20 else 12)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    nnz = int(offsets[-1])
    cols = rng.integers(0, n, nnz, dtype=np.uint32)
    # random values below 2^(bits - 1), every one of which is below r
    coeffs = rng.integers(0, 1 << 64, size=(nnz, limbs), dtype=np.uint64)
    coeffs[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    pick = rng.random(nnz)
    if mix == "r1cs":
        two = (pick >= 0.9) & (pick < 0.95)
        e = rng.integers(1, r.bit_length() - 1, nnz)
        coeffs[two] = 0
        coeffs[two, e[two] // 64] = np.uint64(1) << (e[two] % 64).astype(np.uint64)
    if mix != "general":
        one = pick < (0.8 if mix == "r1cs" else 0.5)
        minus = ~one & (pick < (0.9 if mix == "r1cs" else 2.0))
        coeffs[one] = limbs_of(1, limbs)
        coeffs[minus] = limbs_of(r - 1, limbs)
    return offsets, cols, coeffs


def random_records(curve, n, seed):
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    return a


def load(eng, curve, csr, n, env=None):
    """a handle loaded under the given environment, and the plan of the same load"""
    old = {k: os.environ.pop(k, None) for k in (ENV_NAIVE, ENV_WAVE, ENV_SPLIT)}
    os.environ.update(env or {})
    try:
        plan = libff_amd.plan_fr_matrix(curve, *csr, n, plain=True)
        return eng.fr_matrix_load(curve, *csr, n, plain=True), plan
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def apply_bytes(plan, n_out, rec):
    kept = plan["general"] + plan["plus_one"] + plan["minus_one"]
    return kept * (4 + rec) + plan["general"] * rec + n_out * rec


def median_of(fns):
    """medians of the given calls, alternating, RUNS after WARM"""
    t = [[] for _ in fns]
    for i in range(WARM + RUNS):
        for k, fn in enumerate(fns):
            ms = timed(fn)
            if i >= WARM:
                t[k].append(ms)
    return [(statistics.median(x), min(x), max(x)) for x in t]


def probe(cname, lg, reps):
    curve, n = NAMES[cname], 1 << lg
    eng = libff_amd.Engine(0)
    rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
    mat, _ = load(eng, curve, synthetic(curve, lg, 0), n)
    d_x, d_out = eng.malloc(n * rec), eng.malloc(n * rec)
    eng.h2d(d_x, random_records(curve, n, 1))
    for _ in range(reps):
        eng.fr_matrix_apply_device(mat, d_x, n, d_out, n)
    eng.synchronize()
    print("done")


def main():
    args = sys.argv[1:]
    if args[:1] == ["--probe"]:
        return probe(args[1], int(args[2]), int(args[3]) if len(args) > 3 else 3)
    out = None
    if args[:1] == ["--out"]:
        out, args = open(args[1], "w"), args[2:]
    sweep = "--sweep" in args
    args = [a for a in args if a != "--sweep"]

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    eng = libff_amd.Engine(0)
    emit("one run on one device; medians of %d after %d warm-ups [min max]; (a) .. (d) alternate in one process; the matrix "
         "shape is the issue's assumption, not a survey of circuits" % (RUNS, WARM))
    for spec in args or DEFAULT:
        cname, lgs = spec.split(":")
        curve = NAMES[cname]
        s = libff_amd.sizes(curve, libff_amd.G1)
        rec = s["fr_bytes"]
        g = {0: 5, 1: 22, 2: 15, 3: 7, 4: 10, 5: 17}[curve]
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            seeds = (0, 1, 2) if lg <= 20 else (0,)
            res, naive, plans = [], [], []
            for seed in seeds:
                csr = synthetic(curve, lg, seed)
                m, p = load(eng, curve, csr, n)
                res.append(m)
                plans.append(p)
                naive.append(load(eng, curve, csr, n, {ENV_NAIVE: "1"})[0])
                del csr
            res, naive = (res * 3)[:3], (naive * 3)[:3]
            plans = (plans * 3)[:3]
            d_x = eng.malloc(n * rec)
            d_o = [eng.malloc(n * rec) for _ in range(3)]
            d_aff, d_res = eng.malloc(n * s["affine_bytes"]), eng.malloc(s["g_bytes"])
            eng.h2d(d_x, random_records(curve, n, lg))
            eng.gen_bases_seq_device(curve, libff_amd.G1, 2, n, d_aff)
            eng.synchronize()

            def applies(handles):
                def run():
                    for h, d in zip(handles, d_o):
                        eng.fr_matrix_apply_device(h, d_x, n, d, n)
                    eng.synchronize()
                return run

            def seven():
                for d in d_o:
                    eng.fr_fft_device(curve, d, n, d, inverse=True)
                    eng.fr_fft_device(curve, d, n, d, coset=g)
                eng.fr_fft_device(curve, d_o[0], n, d_o[0], coset=g, inverse=True)
                eng.synchronize()

            def msm():
                eng.msm_device(curve, libff_amd.G1, d_aff, d_x, n, d_res)
                eng.synchronize()

            (a, b, c, d) = median_of([applies(res), applies(naive), seven, msm])
            # the two paths agree, record for record
            got = []
            for handles in (res, naive):
                applies(handles)()
                o = np.zeros((n, rec // 8), dtype=np.uint64)
                eng.d2h(o, d_o[0])
                got.append(o)
            same = bool((got[0] == got[1]).all())
            entries = sum(p["general"] + p["plus_one"] + p["minus_one"] for p in plans)
            traffic = sum(apply_bytes(p, n, rec) for p in plans)
            p = plans[0]
            emit(f"{cname} 2^{lg}: {entries} entries in three matrices ({'three' if len(seeds) == 3 else 'one, applied three times'}); "
                 f"first: general {p['general']} +1 {p['plus_one']} -1 {p['minus_one']}, rows lane/wave/split "
                 f"{p['rows_lane']}/{p['rows_wave']}/{p['rows_split']} at thresholds {p['wave_row']}/{p['split_row']}, longest "
                 f"{p['longest_row']}, chain T = {p['chunk']}, {p['device_bytes'] / 2 ** 20:.1f} MiB resident, {p['launches']} launches")
            emit(f"{cname} 2^{lg}: (a) three applies {a[0]:9.4f} ms [{a[1]:.4f} {a[2]:.4f}] = {entries / a[0] / 1e6:7.2f} G entries/s, "
                 f"{traffic / a[0] / 1e6:7.1f} GB/s effective; (b) naive {b[0]:9.4f} ms [{b[1]:.4f} {b[2]:.4f}], (b)/(a) = {b[0] / a[0]:.2f}; "
                 f"(c) seven transforms {c[0]:9.4f} ms [{c[1]:.4f} {c[2]:.4f}], (a)/(c) = {a[0] / c[0]:.3f}; (d) msm_device G1 "
                 f"{d[0]:9.4f} ms [{d[1]:.4f} {d[2]:.4f}]; paths agree: {same}")
            if cname == "alt_bn128" and lg == 20:
                emit(f"target, alt_bn128 2^20: three applies {a[0]:.4f} ms against seven transforms {c[0]:.4f} ms: "
                     f"{'met' if a[0] <= c[0] else 'MISSED'}")
                eng.set_timing(True)
                eng.fr_matrix_apply_device(res[0], d_x, n, d_o[0], n)
                eng.synchronize()
                ph = eng.get_timings()
                eng.set_timing(False)
                emit(f"alt_bn128 2^20: device time of one apply from the engine's timers: kernels {ph['scatter_ms']:.4f} ms, "
                     f"total {ph['total_ms']:.4f} ms")
                for mix in ("general", "unit"):
                    csr = synthetic(curve, lg, 3, mix)
                    (mr, pr), (mn, _) = load(eng, curve, csr, n), load(eng, curve, csr, n, {ENV_NAIVE: "1"})
                    x, y = median_of([applies([mr]), applies([mn])])
                    k = pr["general"] + pr["plus_one"] + pr["minus_one"]
                    emit(f"alt_bn128 2^20, extreme '{mix}' (general {pr['general']}, +-1 {pr['plus_one'] + pr['minus_one']}): one apply "
                         f"{x[0]:9.4f} ms = {k / x[0] / 1e6:7.2f} G entries/s, {apply_bytes(pr, n, rec) / x[0] / 1e6:7.1f} GB/s "
                         f"effective; naive {y[0]:9.4f} ms, naive/default = {y[0] / x[0]:.2f}")
                    mr.free()
                    mn.free()
                if sweep:
                    csr = synthetic(curve, lg, 0)
                    for wave, split in ((4, 1024), (8, 1024), (16, 1024), (32, 1024), (128, 1024), (32, 128), (32, 256), (32, 512),
                                        (32, 2048), (32, 8192), (32, 65536)):
                        m, p = load(eng, curve, csr, n, {ENV_WAVE: str(wave), ENV_SPLIT: str(split)})
                        (x,) = median_of([applies([m])])
                        emit(f"alt_bn128 2^20, thresholds {p['wave_row']}/{p['split_row']}: rows lane/wave/split "
                             f"{p['rows_lane']}/{p['rows_wave']}/{p['rows_split']}, {p['wave_jobs']} wave jobs, one apply "
                             f"{x[0]:9.4f} ms [{x[1]:.4f} {x[2]:.4f}]")
                        m.free()
            for m in set(res) | set(naive):
                m.free()
            for ptr in [d_x, d_aff, d_res] + d_o:
                eng.free(ptr)
    if out:
        out.close()


if __name__ == "__main__":
    main()
