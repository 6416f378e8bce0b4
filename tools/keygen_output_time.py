#!/usr/bin/env python3
"""Times of the key-generator output path: amdmsm_batch_exp_device against the host entry of another
build of the library, the chain from resident scalars to resident compact affine points both ways, the on-disk encoders
against amdmsm_export_affine_device, and amdmsm_write_points_file against its own phases.

  python tools/keygen_output_time.py [--parent-library PATH/libamdmsm.so] [--log2n 20] [--encode-log2n 22]
                                     [--reps 10] [--warmup 2] [--tmp /dev/shm]

One process, one device; this library and the other build alternate call by call, medians of --reps after --warmup.
Without --parent-library the other build is this library itself (its host entry and its export kernel are the parent's).
Spread = (max - min) of the timed calls.  The two bars: the exponentiation phase of the device entry, and the
uncompressed encoder, may not take longer than the other build's median plus the other build's own spread.  The first
is taken with the host entry's copies (scalars up, results down) made around the device entry's kernel too, so that both
kernels start behind the same traffic; the bare sequence is printed beside it as a report (see main)."""
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
from libff_amd import engine as E  # noqa: E402

WINDOW = 17   # get_exp_window_size at 2^20 scalars for alt_bn128 G1 and bls12_377 G2 (their fixed_base_exp_window_table)


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


def hip_runtime():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise SystemExit("libamdhip64.so not found")


class Timer:
    """device time of what a callable enqueues on the timer's stream"""

    def __init__(self, hip):
        self.hip, self.stream, self.a, self.b = hip, ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(self.stream)) == 0
        assert hip.hipEventCreate(ctypes.byref(self.a)) == 0 and hip.hipEventCreate(ctypes.byref(self.b)) == 0

    def ms(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn(self.stream)
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        out = ctypes.c_float(0)
        assert self.hip.hipEventElapsedTime(ctypes.byref(out), self.a, self.b) == 0
        return out.value


def wall_ms(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    return statistics.median(xs), max(xs) - min(xs)


def alternate(a, b, reps, warmup):
    """a() and b() in turn; the timed values of each"""
    xa, xb = [], []
    for i in range(warmup + reps):
        va, vb = a(), b()
        if i >= warmup:
            xa.append(va)
            xb.append(vb)
    return xa, xb


def line(label, xs, unit="ms"):
    med, spread = stats(xs)
    return f"  {label:<58s} median {med:9.4f} {unit}  spread {spread:8.4f}  (min {min(xs):.4f}, max {max(xs):.4f})"


def plain_scalars(curve, n, seed):
    s = libff_amd.sizes(curve, libff_amd.G1)
    limbs = s["fr_bytes"] // 8
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, limbs), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    top = (s["fr_bits"] - 1) - 64 * (limbs - 1)   # below 2^(bits - 1) < r
    a[:, limbs - 1] &= np.uint64((1 << top) - 1)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--encode-log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tmp", default="/dev/shm")
    a = ap.parse_args()
    new = libff_amd.Engine(0)
    old = other_engine(a.parent_library) if a.parent_library else libff_amd.Engine(0)
    hip = hip_runtime()
    timer = Timer(hip)
    print(f"other build: {a.parent_library or 'this library (no --parent-library)'}; reps {a.reps}, warm-up {a.warmup}")
    ok = True
    n = 1 << a.log2n
    for name, curve, group in (("alt_bn128 G1", libff_amd.ALT_BN128, libff_amd.G1), ("bls12_377 G2", libff_amd.BLS12_377, libff_amd.G2)):
        sz = libff_amd.sizes(curve, group)
        bits = sz["fr_bits"]
        sc = plain_scalars(curve, n, seed=curve)
        g = np.zeros(sz["g_bytes"] // 8, dtype=np.uint64)
        d_one = new.malloc(sz["affine_bytes"])
        d_g = new.malloc(sz["g_bytes"])
        new.gen_bases_seq_device(curve, group, 0, 1, d_one)
        new.export_affine_device(curve, group, d_one, 1, d_g)
        new.synchronize()
        new.d2h(g, d_g)
        d_sc, d_xyz, d_aff = new.malloc(sc.nbytes), new.malloc(n * sz["g_bytes"]), new.malloc(n * sz["affine_bytes"])
        o_sc, o_xyz, o_aff = old.malloc(sc.nbytes), old.malloc(n * sz["g_bytes"]), old.malloc(n * sz["affine_bytes"])
        new.h2d(d_sc, sc)
        old.h2d(o_sc, sc)
        res = np.zeros((n, sz["g_bytes"] // 8), dtype=np.uint64)
        back = np.zeros_like(sc)

        def exp_new(around):
            def run():
                if around:   # the copies the host entry makes around its kernel, made here by hand
                    new.h2d(d_sc, sc)
                new.batch_exp_device(curve, group, bits, WINDOW, g, d_sc, n, d_xyz, scalars_plain=True)
                ms = new.batch_exp_timings()["exp_ms"]
                if around:
                    new.d2h(res, d_xyz)
                return ms
            return run

        def exp_old():
            old.batch_exp(curve, group, bits, WINDOW, g, sc, scalars_plain=True, out=res)
            return old.batch_exp_timings()["exp_ms"]

        # The host entry's kernel starts behind an upload of the scalars and is followed by a download of the results,
        # during which the device idles.  Alternating with it, the bare device entry always starts behind that idle
        # stretch and the host entry behind a kernel: the two do not meet the device in the same state.  The bar is
        # taken with the same copies around both kernels (the timed phase holds the kernel alone either way); the bare
        # sequence is printed beside it.
        for around in (True, False):
            xn, xo = alternate(exp_new(around), exp_old, a.reps, a.warmup)
            (mn, _), (mo, so) = stats(xn), stats(xo)
            verdict = mn <= mo + so
            how = "the host entry's copies around both kernels" if around else "bare device entry (a report)"
            print(f"{name}, n = 2^{a.log2n}, window {WINDOW}: exponentiation phase (timings[2]), {how}")
            print(line("amdmsm_batch_exp_device", xn))
            print(line("amdmsm_batch_exp of the other build, same scalars", xo))
            print(f"  {'bar' if around else 'not the bar'}: {mn:.4f} <= {mo:.4f} + {so:.4f}: {'PASS' if verdict else 'FAIL'}")
            if around:
                ok = ok and verdict

        def chain_new():
            def run():
                new.batch_exp_device(curve, group, bits, WINDOW, g, d_sc, n, d_xyz, scalars_plain=True, out_form=libff_amd.OUT_AFFINE)
                new.import_bases_device(curve, group, d_xyz, sz["g_bytes"], libff_amd.multi_exp_base_form_special, n, d_aff)
            return wall_ms(new, run)

        def chain_old():
            def run():
                old.d2h(back, o_sc)
                old.batch_exp(curve, group, bits, WINDOW, g, back, scalars_plain=True, out=res)
                sp = old.batch_to_special(curve, group, res)
                old.h2d(o_xyz, sp)
                old.import_bases_device(curve, group, o_xyz, sz["g_bytes"], libff_amd.multi_exp_base_form_special, n, o_aff)
            return wall_ms(old, run)

        reps = max(3, a.reps // 2)
        xn, xo = alternate(chain_new, chain_old, reps, 1)
        print(f"{name}, n = 2^{a.log2n}: wall time, resident scalars -> resident compact affine points ({reps} runs; a report)")
        print(line("batch_exp_device(OUT_AFFINE), import_bases_device", xn))
        print(line("download, batch_exp, batch_to_special, upload, import", xo))
        for e, ps in ((new, (d_one, d_g, d_sc, d_xyz, d_aff)), (old, (o_sc, o_xyz, o_aff))):
            e.synchronize()
            for p in ps:
                e.free(p)
        del res, back

    m = 1 << a.encode_log2n
    for name, curve, group in (("alt_bn128 G1", libff_amd.ALT_BN128, libff_amd.G1), ("bw6_761 G1", libff_amd.BW6_761, libff_amd.G1)):
        sz = libff_amd.sizes(curve, group)
        d_aff, d_rec = new.malloc(m * sz["affine_bytes"]), new.malloc(m * sz["g_bytes"])
        o_aff, o_xyz = old.malloc(m * sz["affine_bytes"]), old.malloc(m * sz["g_bytes"])
        new.gen_bases_seq_device(curve, group, 7, m, d_aff)
        old.gen_bases_seq_device(curve, group, 7, m, o_aff)
        new.synchronize()
        old.synchronize()
        enc = lambda c: (lambda: timer.ms(lambda st: new.disk_encode_device(curve, group, d_aff, m, d_rec, compressed=c, stream=st)))
        exp = lambda: timer.ms(lambda st: old.export_affine_device(curve, group, o_aff, m, o_xyz, stream=st))
        xn, xo = alternate(enc(False), exp, a.reps, a.warmup)
        xc, _ = alternate(enc(True), exp, a.reps, a.warmup)
        (mn, _), (mo, so) = stats(xn), stats(xo)
        verdict = mn <= mo + so
        ok = ok and verdict
        gb = m * sz["affine_bytes"] * 2 / 1e9
        print(f"{name}, n = 2^{a.encode_log2n}: encoders against amdmsm_export_affine_device of the other build")
        print(line(f"amdmsm_disk_encode_device ({gb / (mn / 1e3):.0f} GB/s read + written)", xn))
        print(line("amdmsm_disk_encode_device, compressed", xc))
        print(line("amdmsm_export_affine_device of the other build", xo))
        print(f"  bar: {mn:.4f} <= {mo:.4f} + {so:.4f}: {'PASS' if verdict else 'FAIL'}")
        if curve == libff_amd.ALT_BN128:
            path = os.path.join(a.tmp if os.path.isdir(a.tmp) else "/tmp", f"keygen_output_time_{os.getpid()}.bin")
            rec_bytes = m * sz["affine_bytes"]
            host = ctypes.c_void_p()
            assert hip.hipHostMalloc(ctypes.byref(host), ctypes.c_size_t(rec_bytes), 0) == 0
            try:
                wall = [wall_ms(new, lambda: new.write_points_file(curve, group, d_aff, m, path)) for _ in range(a.warmup + a.reps)][a.warmup:]
                copy = [timer.ms(lambda st: hip.hipMemcpyAsync(host, d_rec, ctypes.c_size_t(rec_bytes), 2, st)) for _ in range(a.warmup + a.reps)][a.warmup:]
                buf = (ctypes.c_char * rec_bytes).from_address(host.value)
                fd = os.open(path, os.O_WRONLY)
                hostw = []
                for _ in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    os.pwrite(fd, buf, 0)
                    hostw.append((time.perf_counter() - t0) * 1e3)
                os.close(fd)
                hostw = hostw[a.warmup:]
            finally:
                hip.hipHostFree(host)
                if os.path.exists(path):
                    os.remove(path)
            print(f"{name}, n = 2^{a.encode_log2n}: amdmsm_write_points_file to {os.path.dirname(path)}, chunks of 2^20 (a report)")
            print(line("wall time of the call", wall))
            print(line("encode phase (all records, one launch)", xn))
            print(line("copy phase (device -> pinned host, one copy)", copy))
            print(line("host phase (one pwrite of all records)", hostw))
            print(f"  encode + copy {stats(xn)[0] + stats(copy)[0]:.4f} ms, + host write {stats(xn)[0] + stats(copy)[0] + stats(hostw)[0]:.4f} ms, "
                  f"wall {stats(wall)[0]:.4f} ms")
        for e, ps in ((new, (d_aff, d_rec)), (old, (o_aff, o_xyz))):
            e.synchronize()
            for p in ps:
                e.free(p)
    print("bars:", "PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
