"""Build libff_amd/libamdmsm.so for gfx950 with hipcc (in-tree, no JIT cache).

One translation unit per (curve, group) pair -- msm_group.hip compiled with
-DAMDMSM_GROUP=... -- one per scalar field -- fr_ntt.hip compiled with -DAMDMSM_FR=... --
plus the host engine; the device TUs build in parallel.
Objects are cached under libff_amd/csrc/build/ keyed by source mtimes.
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
SO_PATH = os.path.join(HERE, "libamdmsm.so")

GROUPS = ["alt_bn128_g1", "alt_bn128_g2", "bls12_377_g1", "bls12_377_g2", "bw6_761_g1", "bw6_761_g2",
          "bls12_381_g1", "bls12_381_g2", "mnt4_g1", "mnt4_g2", "mnt6_g1"]
# Per-group code-generation policy (fp.cuh Fp<P, INL>, msm_group.hip), one row per group.  Every group gets
#   AMDMSM_HOT_INLINE  the Montgomery product inlined inside the bucket-accumulation loop
#   AMDMSM_BENCH_BOTH  the inline variants of the throughput probes built too
# and a row adds
#   AMDMSM_ACC_WAVES   waves per SIMD k_accumulate is compiled for (register budget 512 / waves)
#   AMDMSM_ACC_RR      k_accumulate on reduced-radix limbs (rr.cuh: 28 / 29-bit signed limbs, one v_mad_i64_i32 per limb
#                      product and no carry instruction behind it): 1.3x the mixed additions per second of the 32-bit loop on
#                      every pairing field (tools/proto_rr.hip); written for a = 0, so not for the MNT curves
#   AMDMSM_ACC_SPLIT   every Fq2 element split over a pair of lanes in k_accumulate (fp2h.cuh): same multiply-accumulate
#                      count, half the registers per lane
#   AMDMSM_COLD_INLINE products inlined in the cold kernels too (fix-up, bucket reduction, butterfly): fields of fewer than
#                      16 words; no gain for Fq2 / 24 limbs
#   AMDMSM_OVERLAP_OK  the accumulation may run one workgroup per CU short (overlap mode, engine.cpp amdmsm_ctx::bulk_stream;
#                      off by default, it measured slower).  The tail kernels are not capped for it: at 128 registers they
#                      spilled 292 B per lane (profiles/r04_experiments.txt)
def _flags(acc_waves, *on):
    return (["-DAMDMSM_HOT_INLINE=1", "-DAMDMSM_BENCH_BOTH=1"] + [f"-DAMDMSM_{m}=1" for m in on]
            + [f"-DAMDMSM_ACC_WAVES={acc_waves}"])


GROUP_FLAGS = {
    # 9 reduced-radix limbs at three waves (134 registers); cold inline: reduction phase 0.72 -> 0.66 ms at 2^20
    "alt_bn128_g1": _flags(3, "OVERLAP_OK", "COLD_INLINE", "ACC_RR"),
    # lane pairs: 168 VGPRs at three waves, 4.67 -> 4.57 ms at 2^20
    "alt_bn128_g2": _flags(3, "ACC_SPLIT", "ACC_RR"),
    # 14 limbs at two waves; cold inline: reduction phase 2.74 -> 2.10 ms at 2^22
    "bls12_377_g1": _flags(2, "COLD_INLINE", "ACC_RR"),
    # lane pairs: 256 VGPRs + 16 B of scratch at two waves instead of + 440 B, 22.4 -> 18.1 ms at 2^21 (1.86 G madd/s, 0.90
    # of the MAC bound); unconstrained the kernel ran ONE wave per SIMD (28.1 -> 22.9 ms capped at two)
    "bls12_377_g2": _flags(2, "ACC_SPLIT", "ACC_RR"),
    # 28 limbs at two waves (capped at 256 registers: 43.8 -> 35.0 ms at 2^21 against one wave unconstrained)
    "bw6_761_g1": _flags(2, "ACC_RR"),
    "bw6_761_g2": _flags(2, "ACC_RR"),
    "bls12_381_g1": _flags(2, "COLD_INLINE", "ACC_RR"),     # as bls12_377 G1
    "bls12_381_g2": _flags(2, "ACC_SPLIT", "ACC_RR"),       # as bls12_377 G2
    # MNT4-298 / MNT6-298 G1 (a != 0, 10-word field): the 32-bit Montgomery loop at three waves per SIMD
    "mnt4_g1": _flags(3, "COLD_INLINE"),
    # MNT4 G2 (Fq2 = Fq[u]/(u^2 - 17), a' = 34): the 32-bit loop with whole Fq2 elements per lane, two waves per SIMD
    "mnt4_g2": _flags(2),
    "mnt6_g1": _flags(3, "COLD_INLINE"),
}
assert list(GROUP_FLAGS) == GROUPS
# scalar-field units (fr_ntt.hip: the FFT over Fr, its powers and product step), one per curve id
FR_UNITS = {"alt_bn128": 0, "bls12_377": 1, "bw6_761": 2, "bls12_381": 3, "mnt4": 4, "mnt6": 5}
ARCH = "gfx950"
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + INCLUDE, "-I" + CSRC,
          "-Wno-unused-result"]
DEVICE_DEPS = ["msm_group.hip", "group_matrix.inc", "fr_matrix_layout.h", "rr.cuh", "rr_chain.inc", "fp.cuh", "fp2.cuh", "fp2h.cuh", "ec.cuh", "wide.cuh", "wide28.cuh", "mac_chain.inc", "curve_params.h", "group_vtable.h", os.path.join(HERE, "build.py")]
FR_DEPS = ["fr_ntt.hip", "fr_matrix.inc", "fr_matrix_layout.h", "fr_scan.inc", "fr_scan_layout.h", "fr_domain.inc", "mac_chain.inc", "fp.cuh", "curve_params.h", "fr_vtable.h", os.path.join(HERE, "build.py")]
HOST_DEPS = ["engine.cpp", "ffi.cpp", "engine_internal.h", "group_vtable.h", "fr_vtable.h", "fr_matrix_layout.h", "fr_scan_layout.h", "write_plan.h", os.path.join(INCLUDE, "amdmsm.h"),
             os.path.join(INCLUDE, "libff_amd_ffi.h")]


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the amdmsm engine is HIP-only and cannot be built without ROCm")
    return exe


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d if os.path.isabs(d) else os.path.join(CSRC, d)) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s\n%s" % (" ".join(cmd), r.stdout[-4000:], r.stderr[-8000:]))
    return r


def group_flags(g, extra=()):
    """A group's flags with AMDMSM_EXTRA_FLAGS="-DAMDMSM_ACC_WAVES=4 ..." (experiment knobs, the same for every group)
    appended: an experiment flag replaces the group's own setting of the same macro."""
    names = {f.split("=")[0] for f in extra}
    return [f for f in GROUP_FLAGS[g] if f.split("=")[0] not in names] + list(extra)


MAX_BUILD_JOBS = 16


def build_jobs(ntasks):
    """Compilers run at once: MAX_JOBS where set, else the CPUs less one; never more than MAX_BUILD_JOBS -- a shared
    machine reports many more CPUs than a job may use."""
    want = os.environ.get("MAX_JOBS", "")
    n = int(want) if want.isdigit() and int(want) > 0 else (os.cpu_count() or 2) - 1
    return max(1, min(n, ntasks, MAX_BUILD_JOBS))


def build(force=False, verbose=True, jobs=None):
    os.makedirs(OBJ, exist_ok=True)
    cc = hipcc()
    tasks = []
    objs = []
    groups = [g for g in os.environ.get("AMDMSM_GROUPS", ",".join(GROUPS)).split(",") if g]
    extra = os.environ.get("AMDMSM_EXTRA_FLAGS", "").split()
    for g in groups:
        if g not in GROUPS:
            raise RuntimeError(f"unknown group {g!r}")
        o = os.path.join(OBJ, f"group_{g}.o")
        objs.append(o)
        if force or _newer(o, DEVICE_DEPS):
            tasks.append([cc, *COMMON, "-c", os.path.join(CSRC, "msm_group.hip"),
                          f"-DAMDMSM_GROUP={g}", f"-DAMDMSM_VT=vt_{g}", *group_flags(g, extra), "-o", o])
    for c, cid in FR_UNITS.items():
        o = os.path.join(OBJ, f"fr_{c}.o")
        objs.append(o)
        if force or _newer(o, FR_DEPS):
            tasks.append([cc, *COMMON, "-c", os.path.join(CSRC, "fr_ntt.hip"), f"-DAMDMSM_FR={c}_fr",
                          f"-DAMDMSM_FR_VT=frvt_{c}", f"-DAMDMSM_FR_CURVE={cid}", "-o", o])
    # AMDMSM_FFI_NO_REFERENCE_SYMBOLS=1: leave out the reference's own FFI names (<curve>_init / _g1_add /
    # _g1_mul, include/libff_amd_ffi.h) so that the library can sit next to libff-ffi
    no_ref = os.environ.get("AMDMSM_FFI_NO_REFERENCE_SYMBOLS", "0") not in ("", "0")
    for src in ("engine", "ffi"):
        eo = os.path.join(OBJ, f"{src}{'_noref' if no_ref and src == 'ffi' else ''}.o")
        objs.append(eo)
        if force or _newer(eo, HOST_DEPS):
            tasks.append([cc, *COMMON, *(["-DAMDMSM_FFI_NO_REFERENCE_SYMBOLS=1"] if no_ref and src == "ffi" else []),
                          "-x", "hip", "-c", os.path.join(CSRC, f"{src}.cpp"), "-o", eo])
    if tasks:
        if verbose:
            print(f"[libff_amd.build] compiling {len(tasks)} translation unit(s) for {ARCH} ...", flush=True)
        jobs = jobs or build_jobs(len(tasks))
        with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
            list(ex.map(_run, tasks))
    if tasks or not os.path.exists(SO_PATH) or no_ref != os.path.exists(SO_PATH + ".noref"):
        _run([cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-Wl,-soname,libamdmsm.so", "-o", SO_PATH, *objs])
        if no_ref:
            open(SO_PATH + ".noref", "w").close()   # marker: this link carries no reference FFI names
        elif os.path.exists(SO_PATH + ".noref"):
            os.remove(SO_PATH + ".noref")
        if verbose:
            print(f"[libff_amd.build] linked {SO_PATH}", flush=True)
    return SO_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv)
