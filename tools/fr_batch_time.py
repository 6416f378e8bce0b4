#!/usr/bin/env python3
"""Time of the batched Fr transforms and of the one-call witness map against the single calls of another build of the
library (profiles/fr_batch.txt).

  python tools/fr_batch_time.py [--parent-library PATH/libamdmsm.so] [--out profiles/fr_batch.txt]
                                [--skip-witness-map] [--witness-map-log2 16,20,20+10]

This build and the other one (--parent-library: a build of the parent commit; without it this library itself) alternate
in one process, on the same device buffers; medians of 10 after 2 warm-ups, spread = max - min.
  batch      kernels phase of fr_fft_batch_device against the sum of the kernels phases of `batch` calls of the other
             build's fr_fft_device, alt_bn128 and bls12_377, device-resident Montgomery records, out of place.
             Bars: n = 2^16 x 3 and 2^12 x 16: batch < sum - spread of the sum; n = 2^20 x 3: batch <= 3 x single +
             spread of the single; n = 2^8 x 1024: the ratio alone
  map        wall time, from the call to the end of a synchronise, of qap_witness_map_device against the twelve calls
             (three applies, 3 + 3 + 1 domain transforms, a b - c, the division) on the other build; alt_bn128, random
             matrices of 4 entries a row.  Bar: median <= the other's median + its spread
  yardstick  fr_fft_device at 2^20 on both builds: the existing transform has not moved"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libff_amd  # noqa: E402
import libff_amd.engine as E  # noqa: E402

NAMES = {"alt_bn128": 0, "bls12_377": 1}
RUNS, WARM = 10, 2
BATCH_SHAPES = [(16, 3, "faster"), (12, 16, "faster"), (20, 3, "no slower"), (8, 1024, None)]


def other_engine(path):
    """an Engine whose calls go to another build of the library"""
    lib = ctypes.CDLL(path)
    assert lib.amdmsm_abi_version() == E.ABI_VERSION
    lib.amdmsm_strerror.restype = ctypes.c_char_p
    lib.amdmsm_last_error.restype = ctypes.c_char_p
    lib.amdmsm_last_error.argtypes = [ctypes.c_void_p]
    lib.amdmsm_ctx_destroy.restype = None
    lib.amdmsm_ctx_destroy.argtypes = [ctypes.c_void_p]
    e = object.__new__(libff_amd.Engine)
    e.lib, e.device, e.endomorphism, h = lib, 0, 0, ctypes.c_void_p()
    assert lib.amdmsm_ctx_create(0, ctypes.byref(h)) == 0
    e.h = h
    return e


def random_records(curve, n, seed):
    """n canonical Montgomery records: any value below 2^(bits - 1) is one"""
    r = libff_amd.fr_modulus(curve, libff_amd.G1)
    limbs = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, limbs), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << (r.bit_length() - 1 - 64 * (limbs - 1))) - 1)
    return a


def at(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def stats(xs):
    return statistics.median(xs), max(xs) - min(xs)


def alternate(fns):
    """fns: {name: callable returning one figure}; RUNS figures of each after WARM, the callables taking turns"""
    got = {k: [] for k in fns}
    for i in range(WARM + RUNS):
        for k, fn in fns.items():
            v = fn()
            if i >= WARM:
                got[k].append(v)
    return got


def kernels_of(eng, calls):
    """the sum of the kernels phases of the calls, each enqueued with the engine's timers on"""
    total = 0.0
    for call in calls:
        call()
        total += eng.get_timings()["scatter_ms"]
    return total


def wall_of(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3


def batch_section(new, old, emit):
    missed = []
    for cname, curve in NAMES.items():
        rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
        for lg, batch, bar in BATCH_SHAPES:
            n = 1 << lg
            recs = random_records(curve, n * batch, lg + batch)
            d_in, d_out = new.malloc(recs.nbytes), new.malloc(recs.nbytes)
            new.h2d(d_in, recs)
            singles = [lambda v=v: old.fr_fft_device(curve, at(d_in, v * n * rec), n, at(d_out, v * n * rec)) for v in range(batch)]
            for e in (new, old):
                e.set_timing(True)
            try:
                got = alternate({
                    "batch": lambda: kernels_of(new, [lambda: new.fr_fft_batch_device(curve, d_in, n, batch, d_out)]),
                    "singles": lambda: kernels_of(old, singles),
                    "single": lambda: kernels_of(old, singles[:1]),
                })
            finally:
                for e in (new, old):
                    e.set_timing(False)
            (b, bs), (s, ss), (o, os_) = stats(got["batch"]), stats(got["singles"]), stats(got["single"])
            p = libff_amd.plan_fr_fft_batch(curve, n, batch)
            line = (f"batch {cname} n = 2^{lg} x {batch} ({p['workgroups']} workgroups a pass, {p['passes']} passes): batched kernels "
                    f"{b:.4f} ms [spread {bs:.4f}]; other build, {batch} single calls {s:.4f} ms [spread {ss:.4f}], one call {o:.4f} ms "
                    f"[spread {os_:.4f}]; ratio {s / b:.2f}x")
            if bar == "faster":
                ok = b < s - ss
                line += f"; bar batch < sum - spread = {s - ss:.4f}: {'met' if ok else 'MISSED'}"
            elif bar == "no slower":
                ok = b <= 3 * o + os_
                line += f"; bar batch <= 3 x single + spread = {3 * o + os_:.4f}: {'met' if ok else 'MISSED'}"
            else:
                ok = True
                line += "; no bar"
            if not ok:
                missed.append(f"{cname} 2^{lg} x {batch}")
            emit(line)
            new.free(d_in)
            new.free(d_out)
    emit("batch bars: " + ("met everywhere" if not missed else "MISSED at " + "; ".join(missed)))


def random_csr(curve, rows, n_cols, seed, per_row=4):
    rng = np.random.default_rng(seed)
    offsets = (np.arange(rows + 1, dtype=np.uint64) * np.uint64(per_row))
    cols = rng.integers(0, n_cols, size=rows * per_row, dtype=np.uint32)
    return offsets, cols, random_records(curve, rows * per_row, seed + 1)


def map_section(new, old, shapes, emit):
    curve, cname = 0, "alt_bn128"
    rec = libff_amd.sizes(curve, libff_amd.G1)["fr_bytes"]
    g = libff_amd.fr_multiplicative_generator(curve)
    missed = []
    for shape in shapes:
        parts = [int(x) for x in shape.split("+")]
        m = sum(1 << p for p in parts)
        assert libff_amd.fr_domain(curve, m)["m"] == m, shape
        rows, n_cols = m - 1, m // 2
        csr = [random_csr(curve, rows, n_cols, 31 * k + parts[0]) for k in range(3)]
        mats = {e: [e.fr_matrix_load(curve, *c, n_cols) for c in csr] for e in (new, old)}
        z = random_records(curve, n_cols, 5)
        d_z = new.malloc(z.nbytes)
        new.h2d(d_z, z)
        bufs = [new.malloc(m * rec) for _ in range(3)]
        d_h, d_q = new.malloc((m + 1) * rec), new.malloc((m + 1) * rec)

        def one_call():
            new.qap_witness_map_device(curve, *mats[new], d_z, n_cols, m, d_h)

        def twelve_calls():
            for mt, p in zip(mats[old], bufs):
                old.fr_matrix_apply_device(mt, d_z, n_cols, p, m)
            for p in bufs:
                old.fr_domain_fft_device(curve, p, m, p, inverse=True)
                old.fr_domain_fft_device(curve, p, m, p, coset=g)
            old.fr_muladd_device(curve, m, bufs[0], bufs[1], d_q, d_c=bufs[2])
            old.fr_domain_divide_by_z_device(curve, m, d_q, d_q, coset=g)
            old.fr_domain_fft_device(curve, d_q, m, d_q, inverse=True, coset=g)

        wall = alternate({"one": lambda: wall_of(new, one_call), "twelve": lambda: wall_of(old, twelve_calls)})
        h_new, h_old = np.zeros((m, rec // 8), dtype=np.uint64), np.zeros((m, rec // 8), dtype=np.uint64)
        new.d2h(h_new, d_h)
        new.d2h(h_old, d_q)
        same = bool((h_new == h_old).all())
        for e in (new, old):
            e.set_timing(True)
        try:
            def timed_twelve():
                total = 0.0
                for mt, p in zip(mats[old], bufs):
                    total += kernels_of(old, [lambda: old.fr_matrix_apply_device(mt, d_z, n_cols, p, m)])
                for p in bufs:
                    total += kernels_of(old, [lambda: old.fr_domain_fft_device(curve, p, m, p, inverse=True),
                                              lambda: old.fr_domain_fft_device(curve, p, m, p, coset=g)])
                old.fr_muladd_device(curve, m, bufs[0], bufs[1], d_q, d_c=bufs[2])   # no phases of its own: left out on both sides' account
                total += kernels_of(old, [lambda: old.fr_domain_divide_by_z_device(curve, m, d_q, d_q, coset=g),
                                          lambda: old.fr_domain_fft_device(curve, d_q, m, d_q, inverse=True, coset=g)])
                return total
            kern = alternate({"one": lambda: kernels_of(new, [one_call]), "twelve": timed_twelve})
        finally:
            for e in (new, old):
                e.set_timing(False)
        (a, asp), (b, bsp) = stats(wall["one"]), stats(wall["twelve"])
        ok = a <= b + bsp
        if not ok:
            missed.append(shape)
        p = libff_amd.plan_fr_qap_witness_map(curve, m)
        emit(f"map {cname} m = {' + '.join('2^%d' % x for x in parts)} ({rows} rows of 4, {n_cols} columns, workspace "
             f"{p['workspace_bytes'] / 2 ** 20:.1f} MiB): one call {a:.4f} ms [spread {asp:.4f}], kernels {stats(kern['one'])[0]:.4f} ms; "
             f"other build, twelve calls {b:.4f} ms [spread {bsp:.4f}], kernels (a b - c left out) {stats(kern['twelve'])[0]:.4f} ms; "
             f"ratio {b / a:.2f}x; same records: {same}; bar one <= twelve + spread = {b + bsp:.4f}: {'met' if ok else 'MISSED'}")
        for e in (new, old):
            for mt in mats[e]:
                mt.free()
        for p in bufs + [d_z, d_h, d_q]:
            new.free(p)
    emit("map bars: " + ("met everywhere" if not missed else "MISSED at " + "; ".join(missed)))


def yardstick(new, old, emit):
    for cname, curve in NAMES.items():
        n = 1 << 20
        recs = random_records(curve, n, 20)
        d_in, d_out = new.malloc(recs.nbytes), new.malloc(recs.nbytes)
        new.h2d(d_in, recs)
        got = alternate({"this": lambda: wall_of(new, lambda: new.fr_fft_device(curve, d_in, n, d_out)),
                         "other": lambda: wall_of(old, lambda: old.fr_fft_device(curve, d_in, n, d_out))})
        (a, asp), (b, bsp) = stats(got["this"]), stats(got["other"])
        emit(f"yardstick {cname} 2^20: fr_fft_device this build {a:.4f} ms [spread {asp:.4f}], other build {b:.4f} ms [spread {bsp:.4f}]: "
             f"{'within' if abs(a - b) <= bsp else 'OUTSIDE'} the other's spread")
        new.free(d_in)
        new.free(d_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-witness-map", action="store_true")
    ap.add_argument("--witness-map-log2", default="16,20,20+10")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    new = libff_amd.Engine(0)
    old = other_engine(a.parent_library) if a.parent_library else libff_amd.Engine(0)
    emit(f"one run on one device, one process, the builds taking turns; medians of {RUNS} after {WARM} warm-ups, spread = max - min; "
         f"other build: {'a build of the parent commit' if a.parent_library else 'this library (no --parent-library)'}")
    batch_section(new, old, emit)
    if not a.skip_witness_map:
        map_section(new, old, a.witness_map_log2.split(","), emit)
    yardstick(new, old, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
