#!/usr/bin/env python3
"""Time of the scans and of the batch inversion over Fr on device-resident vectors, against the transform over the same
vector and against the one-lane path (profiles/fr_scan.txt).

  python tools/fr_scan_time.py [--out profiles/fr_scan.txt] [alt_bn128:16,20,24 bls12_377:16,20,24 bw6_761:16,20,24]
  python tools/fr_scan_time.py --probe alt_bn128 20 [reps]     inversions and product scans only, for a kernel trace of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fr_scan_time.py --probe ...

Per curve and size n = 2^lg, medians of 10 runs after 2 warm-ups, Montgomery records resident in HBM, out of place, each
time the call and the synchronise behind it, the operations alternating in one process:
  (f) amdmsm_fr_fft_device at the same n, the twiddles resident -- the yardstick, code this change leaves alone;
  (p) the product scan (d_a alone);  (q) the affine scan (d_a and d_b);  (s) prefix sums (d_b alone);
  (i) amdmsm_fr_batch_invert_device;
and with AMDMSM_FR_SCAN_NAIVE=1 (p) and (i) by one lane, 3 runs, up to 2^20 (at 2^24 one lane would walk for a minute).
Then the inversion of a single record against the product scan of a single record -- the same three launches, so the
difference is the one field inversion of the spine -- and a sweep of tile_log2.
The bars: (p) <= (f) for alt_bn128 at 2^20; (i) <= (f) at 2^24; (q) is expected within 1.5 x (p)."""
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
NAIVE_MAX_LG = 20


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def random_records(curve, n, seed):
    """n canonical, nonzero Montgomery records: any value below 2^(bits - 1) is canonical"""
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    a[:, 0] |= np.uint64(1)
    return a


class Case:
    def __init__(self, eng, curve, n, seed):
        self.eng, self.curve, self.n = eng, curve, n
        recs = random_records(curve, n, seed)
        self.bufs = [eng.malloc(recs.nbytes) for _ in range(3)]
        self.d_a, self.d_b, self.d_out = self.bufs
        eng.h2d(self.d_a, recs)
        eng.h2d(self.d_b, random_records(curve, n, seed + 1))
        eng.synchronize()

    def free(self):
        for b in self.bufs:
            self.eng.free(b)

    def fft(self):
        self.eng.fr_fft_device(self.curve, self.d_a, self.n, self.d_out)
        self.eng.synchronize()

    def product(self, tile=0):
        self.eng.fr_scan_device(self.curve, self.n, self.d_out, self.d_a, tile_log2=tile)
        self.eng.synchronize()

    def affine(self, tile=0):
        self.eng.fr_scan_device(self.curve, self.n, self.d_out, self.d_a, self.d_b, tile_log2=tile)
        self.eng.synchronize()

    def sums(self, tile=0):
        self.eng.fr_scan_device(self.curve, self.n, self.d_out, None, self.d_b, tile_log2=tile)
        self.eng.synchronize()

    def invert(self, tile=0):
        self.eng.fr_batch_invert_device(self.curve, self.n, self.d_a, self.d_out, tile_log2=tile)
        self.eng.synchronize()


def alternate(fns, runs=RUNS, warm=WARM):
    """medians (and the samples) of the functions run in turn"""
    samples = [[] for _ in fns]
    for i in range(warm + runs):
        for k, fn in enumerate(fns):
            t = timed(fn)
            if i >= warm:
                samples[k].append(t)
    return [statistics.median(s) for s in samples], samples


def naive_env(on):
    if on:
        os.environ["AMDMSM_FR_SCAN_NAIVE"] = "1"
    else:
        os.environ.pop("AMDMSM_FR_SCAN_NAIVE", None)


def probe(cname, lg, reps):
    eng = libff_amd.Engine(0)
    c = Case(eng, NAMES[cname], 1 << lg, 1)
    for _ in range(reps):
        c.invert()
        c.product()
        c.affine()
    c.free()
    print("done")


def main():
    args = sys.argv[1:]
    if args[:1] == ["--probe"]:
        return probe(args[1], int(args[2]), int(args[3]) if len(args) > 3 else 3)
    out = None
    if args[:1] == ["--out"]:
        out, args = open(args[1], "w"), args[2:]

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    naive_env(False)
    eng = libff_amd.Engine(0)
    emit("one run on one device; medians of %d after %d warm-ups; the operations alternate in one process" % (RUNS, WARM))
    bars = []
    for spec in args or DEFAULT:
        cname, lgs = spec.split(":")
        curve = NAMES[cname]
        rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            try:
                libff_amd.fr_root_of_unity(curve, n)
            except ValueError:
                emit(f"{cname} 2^{lg}: above the field's 2-adicity, left out")
                continue
            c = Case(eng, curve, n, lg)
            p = libff_amd.plan_fr_scan(curve, n)
            (f, pr, af, su, iv), smp = alternate([c.fft, c.product, c.affine, c.sums, c.invert])
            spread = lambda s: f"[min {min(s):.4f} max {max(s):.4f}]"
            moved = lambda vectors: vectors * n * rec / 1e6   # MB: reduce reads, apply reads and writes
            emit(f"{cname} 2^{lg}: tile 2^{p['tile'].bit_length() - 1}, workspace {p['workspace_bytes'] / 2 ** 10:.0f} KiB; "
                 f"(f) fr_fft_device {f:9.4f} ms {spread(smp[0])}; "
                 f"(p) product scan {pr:9.4f} ms {spread(smp[1])} = {pr / f:.3f} (f), {moved(3) / pr:6.1f} GB/s over 3 record moves; "
                 f"(q) affine scan {af:9.4f} ms {spread(smp[2])} = {af / pr:.3f} (p), {moved(5) / af:6.1f} GB/s over 5; "
                 f"(s) prefix sums {su:9.4f} ms {spread(smp[3])}, {moved(3) / su:6.1f} GB/s over 3; "
                 f"(i) batch inversion {iv:9.4f} ms {spread(smp[4])} = {iv / f:.3f} (f), {moved(3) / iv:6.1f} GB/s over 3")
            eng.set_timing(True)
            c.invert()
            ph = eng.get_timings()
            eng.set_timing(False)
            emit(f"{cname} 2^{lg}: phases of a timed (i), {ph['total_ms']:.4f} ms: kernels {ph['scatter_ms']:.4f}")
            if cname == "alt_bn128" and lg == 20:
                bars.append(("product scan, alt_bn128 2^20, at most one fr_fft", pr, f))
            if lg == 24:
                bars.append((f"batch inversion, {cname} 2^24, at most one fr_fft", iv, f))
            if lg <= NAIVE_MAX_LG:
                naive_env(True)
                (npr, niv), _ = alternate([c.product, c.invert], runs=3, warm=1)
                naive_env(False)
                emit(f"{cname} 2^{lg}: one lane (AMDMSM_FR_SCAN_NAIVE=1, 3 runs): product scan {npr:10.3f} ms = {npr / pr:7.1f} x (p); "
                     f"batch inversion {niv:10.3f} ms = {niv / iv:7.1f} x (i)")
            else:
                emit(f"{cname} 2^{lg}: one lane: not measured")
            if lg in (20, 24) and cname == "alt_bn128":
                for tl in range(p["tile_min"], p["tile_max"] + 1):
                    (tp, ta, ti), _ = alternate([lambda: c.product(tl), lambda: c.affine(tl), lambda: c.invert(tl)], runs=5, warm=1)
                    emit(f"{cname} 2^{lg}: tile_log2 = {tl}: product scan {tp:9.4f} ms, affine scan {ta:9.4f} ms, batch inversion {ti:9.4f} ms")
            c.free()
        # the one inversion: a single record, against a product scan of a single record (the same three launches)
        one = Case(eng, curve, 1, 99)
        (i1, p1), _ = alternate([one.invert, one.product], runs=20, warm=3)
        emit(f"{cname} n = 1: batch inversion {i1:.4f} ms, product scan {p1:.4f} ms: the spine's field inversion, one lane, about "
             f"{i1 - p1:.4f} ms")
        one.free()
    for what, got, yard in bars:
        emit(f"bar, {what}: {got:.4f} ms against {yard:.4f} ms: {'met' if got <= yard else 'MISSED'} ({got / yard:.3f})")
    if out:
        out.close()


if __name__ == "__main__":
    main()
