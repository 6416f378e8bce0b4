#!/usr/bin/env python3
"""Time of the transforms over a step radix-2 domain and of the division by Z on device-resident vectors, against the
radix-2 transform they are built around (profiles/fr_domain.txt).

  python tools/fr_domain_time.py [--out profiles/fr_domain.txt] [alt_bn128:20+19,20+10,20+0 bls12_377:20+19,20+10,20+0]
  python tools/fr_domain_time.py --yardstick [alt_bn128:20 bls12_377:20]     amdmsm_fr_fft_device alone: the figure to
      compare between two builds (AMDMSM_LIBRARY names another build of the same ABI)

Per curve and m = 2^b + 2^s, Montgomery records, out of place, medians of 10 runs after 2 warm-ups, one process:
  the call and the synchronise behind it of the forward, the inverse, the coset and the inverse coset transform and of
  the division, and of the yardstick amdmsm_fr_fft_device at n = B and n = S -- kernels this change leaves as the parent
  has them (tools/asm_identity.py);
  the kernels phase of the same calls from the engine's timers (a run of their own, medians again), and from them
      sweep = kernels(domain transform) - passes(n = B) - passes(n = S):   the fold, or the merge with its row 0
      pass  = passes(n = 2 B) / its number of passes:                      one global pass of k_fr_fft_pass over 2 B records
The bar: sweep <= pass, for every form and shape."""
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
DEFAULT = ["alt_bn128:20+19,20+10,20+0", "bls12_377:20+19,20+10,20+0"]


def random_records(curve, n, seed):
    """n canonical Montgomery records: any value below 2^(bits - 1) is one"""
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    return a


def measure(eng, fn):
    """(median wall ms, min, max, median kernels-phase ms) of fn, which enqueues one call"""
    def once():
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    wall = [once() for _ in range(WARM + RUNS)][WARM:]
    eng.set_timing(True)
    try:
        kern = []
        for _ in range(RUNS):
            fn()
            kern.append(eng.get_timings()["scatter_ms"])
    finally:
        eng.set_timing(False)
    return statistics.median(wall), min(wall), max(wall), statistics.median(kern)


def yardstick(eng, specs, emit):
    for spec in specs:
        cname, lgs = spec.split(":")
        curve = NAMES[cname]
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            recs = random_records(curve, n, lg)
            d_in, d_out = eng.malloc(recs.nbytes), eng.malloc(recs.nbytes)
            eng.h2d(d_in, recs)
            w, lo, hi, k = measure(eng, lambda: eng.fr_fft_device(curve, d_in, n, d_out))
            emit(f"yardstick {cname} 2^{lg}: fr_fft_device {w:.4f} ms [min {lo:.4f} max {hi:.4f}], passes phase {k:.4f} ms")
            eng.free(d_in)
            eng.free(d_out)


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
    if args[:1] == ["--yardstick"]:
        emit("one run on one device; medians of %d after %d warm-ups; library %s" % (RUNS, WARM, libff_amd.engine.SO_PATH))
        return yardstick(eng, args[1:] or ["alt_bn128:20", "bls12_377:20"], emit)
    emit("one run on one device; medians of %d after %d warm-ups; one process" % (RUNS, WARM))
    missed = []
    for spec in args or DEFAULT:
        cname, shapes = spec.split(":")
        curve = NAMES[cname]
        g = libff_amd.fr_multiplicative_generator(curve)
        rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
        for shape in shapes.split(","):
            lb, ls = (int(x) for x in shape.split("+"))
            B, S = 1 << lb, 1 << ls
            m = B + S
            d = libff_amd.fr_domain(curve, m)
            assert (d["kind"], d["m"], d["B"], d["S"]) == (libff_amd.DOMAIN_STEP_RADIX2, m, B, S), d
            recs = random_records(curve, 2 * B, lb + ls)
            d_in, d_out = eng.malloc(recs.nbytes), eng.malloc(recs.nbytes)
            eng.h2d(d_in, recs)
            fft = {n: measure(eng, lambda n=n: eng.fr_fft_device(curve, d_in, n, d_out)) for n in (B, S, 2 * B)}
            passes = libff_amd.plan_fr_fft(curve, 2 * B)["passes"]
            one_pass = fft[2 * B][3] / passes
            emit(f"{cname} m = 2^{lb} + 2^{ls} (K = {B // S}), workspace {d['workspace_bytes'] / 2 ** 20:.1f} MiB; yardsticks: "
                 f"fr_fft_device n = B {fft[B][0]:.4f} ms (passes {fft[B][3]:.4f}), n = S {fft[S][0]:.4f} ms (passes {fft[S][3]:.4f}), "
                 f"n = 2B passes {fft[2 * B][3]:.4f} ms in {passes} = {one_pass:.4f} ms a pass, {4 * B * rec / one_pass / 1e6:.0f} GB/s")
            forms = [("forward", {}), ("inverse", {"inverse": True}), ("coset", {"coset": g}),
                     ("inverse coset", {"inverse": True, "coset": g})]
            for name, kw in forms:
                w, lo, hi, k = measure(eng, lambda kw=kw: eng.fr_domain_fft_device(curve, d_in, m, d_out, **kw))
                sweep = k - fft[B][3] - fft[S][3]
                ok = sweep <= one_pass
                if not ok:
                    missed.append(f"{cname} 2^{lb} + 2^{ls} {name}")
                emit(f"  {name:14s} {w:9.4f} ms [min {lo:.4f} max {hi:.4f}]; kernels {k:.4f} ms, of them the "
                     f"{'merge' if 'inverse' in kw else 'fold'} {sweep:.4f} ms = {sweep / one_pass:.2f} of a pass: {'met' if ok else 'MISSED'}")
            w, lo, hi, k = measure(eng, lambda: eng.fr_domain_divide_by_z_device(curve, m, d_in, d_out, coset=g))
            emit(f"  {'divide by Z':14s} {w:9.4f} ms [min {lo:.4f} max {hi:.4f}]; kernels (inversion of {B // S} denominators and the "
                 f"products) {k:.4f} ms = {k / one_pass:.2f} of a pass")
            eng.free(d_in)
            eng.free(d_out)
    emit("bar (fold or merge <= one global pass over 2B records): " + ("met everywhere" if not missed else "MISSED at " + "; ".join(missed)))
    yardstick(eng, ["alt_bn128:20", "bls12_377:20"], emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
