#!/usr/bin/env python3
"""Time of the sparse matrix times point vector on device-resident points (amdmsm_group_matrix_apply_device) against the
route there was before and its two yardsticks (profiles/group_matrix.txt).

  python tools/group_matrix_time.py [--out profiles/group_matrix.txt] [alt_bn128_g1:16,20 bw6_761_g1:16 ...]

The workload is the synthetic R1CS matrix of tools/fr_matrix_time.py (its shape is that issue's assumption, not a survey
of circuits), loaded transposed: n = 2^lg constraints and as many variables, so the handle has n rows over n points --
the shape of a Groth16 query from the Lagrange form of a ceremony's powers.  Two mixes: 'r1cs' (eight coefficients in ten
1, one in ten r - 1, the rest general) and 'unit' (every coefficient 1 or r - 1).  Points are (2 + i) G made on the
device.  Per group, size and mix, medians of 10 runs after 2 warm-ups, each run the call and the synchronise behind it,
the routes alternating in one process:
  (new) amdmsm_group_matrix_apply_device, AMDMSM_OUT_AFFINE, automatic chunks;
  (1)   the only route before: amdmsm_msm_device_segments over the nnz pre-gathered bases and coefficients, one segment
        per row, AMDMSM_OUT_AFFINE.  The gather on the host and its upload are not timed, which favours it;
  (2)   amdmsm_scalar_mul_vec_device over as many elements as the matrix has general entries (r1cs mix);
  (3)   amdmsm_madd_bench_device: its mixed additions per second (operands in registers) times the kept entries.
The two routes' records are compared bit for bit.  The phases of (new) come from the engine's timers.
The gate: on the unit mix every run of (new) is below every run of (1)."""
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import libff_amd  # noqa: E402
from fr_matrix_time import NAMES, RUNS, WARM, synthetic, timed  # noqa: E402

DEFAULT = ["alt_bn128_g1:16,20", "alt_bn128_g2:16,20", "bls12_381_g1:16,20", "bw6_761_g1:16"]


def runs_of(fns):
    """the times of the given calls, alternating, RUNS after WARM"""
    t = [[] for _ in fns]
    for i in range(WARM + RUNS):
        for k, fn in enumerate(fns):
            ms = timed(fn)
            if i >= WARM:
                t[k].append(ms)
    return t


def fmt(x):
    return f"{statistics.median(x):10.4f} ms [{min(x):.4f} {max(x):.4f}]"


def transposed_terms(offsets, cols, n):
    """the transpose's rows as segments: (segment offsets, the row of M behind every term, the entry of M behind it)"""
    lens = np.diff(offsets).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.uint32), lens)
    order = np.argsort(cols, kind="stable")
    seg = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(cols, minlength=n), out=seg[1:])
    return seg, rows[order], order


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
    emit("one run on one device; medians of %d after %d warm-ups [min max]; the routes alternate in one process; the matrix "
         "shape is an assumption, not a survey of circuits" % (RUNS, WARM))
    for spec in args or DEFAULT:
        gname, lgs = spec.split(":")
        cname, gid = gname.rsplit("_g", 1)
        curve, group = NAMES[cname], int(gid)
        s = libff_amd.sizes(curve, group)
        aff, xyz, fr = s["affine_bytes"], s["g_bytes"], s["fr_bytes"]
        for lg in (int(x) for x in lgs.split(",")):
            n = 1 << lg
            d_pts, d_new, d_old = eng.malloc(n * aff), eng.malloc(n * xyz), eng.malloc(n * xyz)
            eng.gen_bases_seq_device(curve, group, 2, n, d_pts)
            eng.synchronize()
            pts = np.zeros((n, aff // 8), dtype=np.uint64)
            eng.d2h(pts, d_pts)
            for mix in ("unit", "r1cs"):
                offsets, cols, coeffs = synthetic(curve, lg, 0, mix)
                mat = eng.fr_matrix_load_transposed(curve, offsets, cols, coeffs, n, plain=True)
                plan = eng.plan_group_matrix(mat, group)
                kept, gen = plan["general"] + plan["plus_minus_one"], plan["general"]
                seg, term_rows, term_src = transposed_terms(offsets, cols, n)
                nnz = int(seg[-1])
                d_bases, d_coef = eng.malloc(nnz * aff), eng.malloc(nnz * fr)
                eng.h2d(d_bases, pts[term_rows])
                eng.h2d(d_coef, coeffs[term_src])
                del term_rows, term_src, coeffs, cols, offsets

                def new():
                    eng.group_matrix_apply_device(mat, group, d_pts, n, d_new, out_form=libff_amd.OUT_AFFINE)
                    eng.synchronize()

                def old():
                    eng.msm_device_segments(curve, group, d_bases, nnz, d_coef, nnz, seg, d_old, out_form=libff_amd.OUT_AFFINE,
                                            scalars_plain=True)
                    eng.synchronize()

                fns = [new, old]
                if mix == "r1cs":
                    assert 0 < gen <= n
                    d_sc, d_smv = eng.malloc(gen * fr), eng.malloc(gen * xyz)
                    eng.h2d(d_sc, np.random.default_rng(lg).integers(0, 1 << 62, size=(gen, fr // 8), dtype=np.uint64))

                    def smv():
                        eng.scalar_mul_vec_device(curve, group, d_pts, d_sc, gen, d_smv, out_form=libff_amd.OUT_AFFINE,
                                                  scalars_plain=True)
                        eng.synchronize()

                    fns.append(smv)
                t = runs_of(fns)
                got = [np.zeros((n, xyz // 8), dtype=np.uint64) for _ in range(2)]
                eng.d2h(got[0], d_new)
                eng.d2h(got[1], d_old)
                same = bool((got[0] == got[1]).all())
                # the mixed-addition rate with operands in registers
                lanes, iters, ms = 1 << 18, 64, ctypes.c_float()
                rate = []
                for _ in range(1 + 5):
                    eng._check(eng.lib.amdmsm_madd_bench_device(eng.h, curve, group, d_pts, d_old, ctypes.c_size_t(min(lanes, n)), iters, 2,
                                                                ctypes.byref(ms)), "amdmsm_madd_bench_device")
                    eng.synchronize()
                    rate.append(min(lanes, n) * iters / ms.value / 1e6)
                rate = statistics.median(rate[1:])
                eng.set_timing(True)
                new()
                ph = eng.get_timings()
                eng.set_timing(False)
                tag = f"{gname} 2^{lg} {mix:4s}"
                emit(f"{tag}: {kept} entries kept, {gen} general, {plan['wave_jobs']} wave jobs, {plan['partials']} partials, "
                     f"{plan['chunks']} chunk(s), {plan['launches']} launches, workspace {plan['workspace_bytes'] / 2 ** 20:.1f} MiB")
                emit(f"{tag}: (new) {fmt(t[0])} = {kept / statistics.median(t[0]) / 1e6:7.3f} G entries/s; (1) segments {fmt(t[1])}, "
                     f"(1)/(new) = {statistics.median(t[1]) / statistics.median(t[0]):.2f}; routes agree: {same}")
                emit(f"{tag}: phases of (new): general pass {ph['scatter_ms']:.4f} ms, accumulation and combine {ph['accumulate_ms']:.4f} ms, "
                     f"normalisation {ph['reduce_ms']:.4f} ms, total {ph['total_ms']:.4f} ms; (3) madd rate {rate:.3f} G/s x {kept} entries = "
                     f"{kept / rate / 1e6:.4f} ms, accumulation / (3) = {ph['accumulate_ms'] / (kept / rate / 1e6):.2f}")
                if mix == "unit":
                    emit(f"{tag}: gate, every run of (new) below every run of (1): max (new) {max(t[0]):.4f} ms, min (1) {min(t[1]):.4f} ms: "
                         f"{'met' if max(t[0]) < min(t[1]) else 'MISSED'}")
                else:
                    emit(f"{tag}: (2) scalar_mul_vec over {gen} elements {fmt(t[2])}; general pass / (2) = "
                         f"{ph['scatter_ms'] / statistics.median(t[2]):.2f}")
                    eng.free(d_sc)
                    eng.free(d_smv)
                mat.free()
                eng.free(d_bases)
                eng.free(d_coef)
            for p in (d_pts, d_new, d_old):
                eng.free(p)
    if out:
        out.close()


if __name__ == "__main__":
    main()
