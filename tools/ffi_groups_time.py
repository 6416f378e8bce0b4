#!/usr/bin/env python3
"""amdmsm_ffi_last_timings of the FFI calls, one-shot (<curve>_g?_multiexp) and loaded (amdmsm_ffi_bases_load +
amdmsm_ffi_multiexp_loaded), for chosen groups and sizes (profiles/ffi_groups.txt).

  python tools/ffi_groups_time.py 16,20 bls12_381_g1 bls12_381_g2 mnt4_g1 mnt4_g2 mnt6_g1 +bls12_377_g1 +mnt4_g2

A leading + also times the loaded call for that group.  Bases are (5 + i) G made on the device and rewritten in the
wire format; scalars are random below 2^(8 (fr_bytes - 1)) (MNT: 2^296).  Three repetitions per line, all printed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libff_amd  # noqa: E402
from libff_amd import ffi  # noqa: E402

NAMES = {"alt_bn128": 0, "bls12_377": 1, "bw6_761": 2, "bls12_381": 3, "mnt4": 4, "mnt6": 5}


def wire_bases(eng, curve, group, n):
    s = libff_amd.sizes(curve, group)
    deg = 2 if (group == 2 and curve != libff_amd.BW6_761) else 1
    cw = s["affine_bytes"] // 16          # 64-bit words per coordinate
    fw_ = cw // deg                       # per Fq component
    am = np.ascontiguousarray(eng.gen_bases_seq(curve, group, n, first=5, as_xyz=False)).reshape(2 * n, cw)
    one = np.zeros_like(am)
    one[:, 0] = 1
    plain = eng.field_op(curve, group, 0, am, one).reshape(2 * n, deg, fw_)   # Montgomery product with 1: plain value
    be = np.ascontiguousarray(plain[:, ::-1, ::-1]).view(np.uint8).reshape(2 * n, deg, fw_, 8)[..., ::-1]
    return np.ascontiguousarray(be).reshape(-1)


def main():
    lgs = [int(x) for x in sys.argv[1].split(",")]
    eng = libff_amd.Engine(0)
    for arg in sys.argv[2:]:
        loaded = arg.startswith("+")
        name = arg.lstrip("+")
        cname, g = name.rsplit("_g", 1)
        curve, group = NAMES[cname], int(g)
        es = ffi.element_sizes(curve, group)
        for lg in lgs:
            n = 1 << lg
            bases = wire_bases(eng, curve, group, n)
            sc = np.random.default_rng(78).integers(0, 256, size=(n, es["fr_bytes"]), dtype=np.uint8)
            sc[:, : (3 if es["fr_bytes"] == 40 else 1)] = 0
            sc = sc.reshape(-1)
            ref = None
            for rep in range(3):
                t0 = time.perf_counter()
                out = ffi.multiexp(curve, group, bases, sc)
                dt = (time.perf_counter() - t0) * 1e3
                assert out is not None and (ref is None or out == ref)
                ref = out
                ms = ffi.last_timings()
                print(f"{name} 2^{lg} one-shot rep {rep}: call {dt:8.2f} ms  [0] upload {ms[0]:7.2f}  "
                      f"[1] decode+validate {ms[1]:8.2f}  [2] msm+encode {ms[2]:7.2f}", flush=True)
            if loaded:
                t0 = time.perf_counter()
                h = ffi.load_bases(curve, group, bases)
                assert h is not None
                dt = (time.perf_counter() - t0) * 1e3
                ms = ffi.last_timings()
                print(f"{name} 2^{lg} bases_load      : call {dt:8.2f} ms  [0] upload {ms[0]:7.2f}  "
                      f"[1] decode+validate {ms[1]:8.2f}  [2] -", flush=True)
                for rep in range(3):
                    t0 = time.perf_counter()
                    out = ffi.multiexp_loaded(h, sc)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert out == ref
                    ms = ffi.last_timings()
                    print(f"{name} 2^{lg} loaded   rep {rep}: call {dt:8.2f} ms  [0] scalar upload {ms[0]:7.2f}  "
                          f"[1] scalar decode {ms[1]:8.2f}  [2] msm+encode {ms[2]:7.2f}", flush=True)
                assert ffi.free_bases(h)


if __name__ == "__main__":
    main()
