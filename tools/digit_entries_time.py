"""Sort phase of the entries whose digit pass is k_sort_digits_short<K> or k_sort_digits_sel, beside the plain entry:
alt_bn128 G1 at 2^16, 2^20 and 2^22 points, device-resident bases and scalars, timing on, each entry 18 times with the
first 3 dropped; prints the median (minimum) of phases_ms.scatter_ms and the median of total_ms.

    python tools/digit_entries_time.py
    AMDMSM_LIBRARY=<library of another build> python tools/digit_entries_time.py      # the same with that build

u8 / u32: msm_device_short on packed bytes / 32-bit words; sel: msm_device_batch_items, one item whose scalars are a
random permutation index into a shared vector of plain scalars; plain: msm_device on the same plain scalars.
Raw output: profiles/digit_pass_and_step_gaps.txt section 9."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libff_amd  # noqa: E402


def main():
    eng = libff_amd.Engine(0)
    eng.set_timing(True)
    rng = np.random.default_rng(3)
    s = libff_amd.sizes(0, 1)
    fl = s["fr_bytes"] // 8

    def put(arr):
        arr = np.ascontiguousarray(arr)
        p = eng.malloc(arr.nbytes)
        eng.h2d(p, arr)
        return p

    def timed(f):
        out = []
        for i in range(18):
            f()
            eng.synchronize()
            ms = eng.get_timings()
            if i >= 3:
                out.append((ms["scatter_ms"], ms["total_ms"]))
        return "sort %.4f (min %.4f) total %.4f" % (statistics.median(x[0] for x in out), min(x[0] for x in out), statistics.median(x[1] for x in out))

    for lg in (16, 20, 22):
        n = 1 << lg
        d_aff = eng.malloc(n * s["affine_bytes"])
        eng.gen_bases_seq_device(0, 1, 1, n, d_aff)
        d_out = eng.malloc(s["g_bytes"])
        d_u8 = put(rng.integers(0, 256, n).astype(np.uint8))
        d_u32 = put(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        sc = rng.integers(0, 1 << 63, size=(n, fl), dtype=np.uint64)
        sc[:, -1] &= np.uint64((1 << 58) - 1)
        d_sc = put(sc)
        d_idx = put(rng.permutation(n).astype(np.uint32))
        print("2^%d u8   " % lg, timed(lambda: eng.msm_device_short(0, 1, d_aff, d_u8, 1, n, d_out)))
        print("2^%d u32  " % lg, timed(lambda: eng.msm_device_short(0, 1, d_aff, d_u32, 4, n, d_out)))
        print("2^%d sel  " % lg, timed(lambda: eng.msm_device_batch_items(0, 1, [dict(bases=d_aff.value, n=n, index=d_idx.value, out=d_out.value)], d_sc.value, n, scalars_plain=True)))
        print("2^%d plain" % lg, timed(lambda: eng.msm_device(0, 1, d_aff, d_sc, n, d_out, scalars_plain=True)))
        for p in (d_aff, d_out, d_u8, d_u32, d_sc, d_idx):
            eng.free(p)


if __name__ == "__main__":
    main()
