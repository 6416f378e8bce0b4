#!/usr/bin/env python3
"""Generate tests/golden/ffi_mnt.npz: what the reference's FFI codecs and multi_exp do for MNT4-298 G1 / G2 and
MNT6-298 G1, the groups libff-ffi itself has no entry points for.

Runs ONLY where the reference is mounted (LIBFF_REFERENCE, default /root/reference): the driver below is compiled
against the reference's MNT sources, in a temporary directory, with the flags of oracle/build_ref.sh.  It reads and
writes every element through ffi::group_element_read / group_element_write / field_element_read / field_element_write
(ffi/ffi_serialization.tcc) and sums with libff::multi_exp.  The file holds data only -- wire-format byte strings and
the bool each read returned.  Per group <g> in mnt4_g1, mnt4_g2, mnt6_g1:

  <g>/bases (64, E)  <g>/scalars (64, 40)  <g>/msm_out (E,)     bases (17 + i) G, scalars 1 / (1000 + i)
  <g>/add_a, add_b, add_out (6, E)      P + Q, P + P, P + (-P), P + 0, 0 + Q, 0 + 0
  <g>/mul_p (4, E)  mul_s (4, 40)  mul_out (4, E)   s = 1 / 7, 0, 1, r - 1
  <g>/curve_points (k, E)  <g>/curve_points_ok (k,)   points found by solving the curve equation for y (x = 2, 3, ...):
      on the curve, group_element_read's verdict recorded; for mnt4_g2 followed by their multiples by the cofactor h,
      which the reference accepts (the twist's order is h r: a random point of it lies outside the order-r subgroup)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LIBFF_REFERENCE", "/root/reference")
GMPINC = os.path.join(ROOT, "oracle", "_ref", "gmpinc")   # staged by oracle/build_ref.sh

DRIVER = r"""
#include <cstdio>
#include <vector>
#include <libff/algebra/curves/mnt/mnt4/mnt4_pp.hpp>
#include <libff/algebra/curves/mnt/mnt6/mnt6_pp.hpp>
#include <libff/algebra/scalar_multiplication/multiexp.hpp>
#include <ffi/ffi_serialization.hpp>

using namespace libff;

static void put(const char *g, const char *key, const std::vector<unsigned char> &b)
{
    printf("%s/%s ", g, key);
    for (unsigned char c : b) printf("%02x", c);
    printf("\n");
}
template<typename G> static std::vector<unsigned char> enc(const G &p)
{
    std::vector<unsigned char> b(2 * sizeof(p.X));
    if (!ffi::group_element_write(p, b.data(), b.size())) abort();
    return b;
}
template<typename F> static std::vector<unsigned char> enc_f(const F &s)
{
    std::vector<unsigned char> b(sizeof(s));
    if (!ffi::field_element_write(s, b.data(), b.size())) abort();
    return b;
}
// every operand goes through the reference's read, as <curve>_g1_add / _g1_mul do (ffi.cpp:16-54)
template<typename G> static G rd(const G &p, bool &ok)
{
    std::vector<unsigned char> b = enc(p);
    G q;
    ok = ffi::group_element_read(q, b.data(), b.size());
    return q;
}

template<typename G, typename Fr, typename Fc> static void emit(const char *g, bool with_cofactor)
{
    const size_t n = 64;
    std::vector<G> bases;
    std::vector<Fr> scalars;
    bool ok;
    for (size_t i = 0; i < n; ++i) {
        G p = Fr((long)(17 + i)) * G::one();
        p.to_special();
        bases.push_back(rd(p, ok));
        if (!ok) abort();
        std::vector<unsigned char> sb = enc_f(Fr((long)(1000 + i)).inverse());
        Fr s;
        if (!ffi::field_element_read(s, sb.data(), sb.size())) abort();
        scalars.push_back(s);
        put(g, "bases", enc(bases[i]));
        put(g, "scalars", sb);
    }
    const G sum = multi_exp<G, Fr, multi_exp_method_BDLO12_signed, multi_exp_base_form_special>(
        bases.cbegin(), bases.cend(), scalars.cbegin(), scalars.cend(), 1);
    put(g, "msm_out", enc(sum));

    const G P = bases[3], Q = bases[9], Z = G::zero();
    const G pairs[6][2] = {{P, Q}, {P, P}, {P, -P}, {P, Z}, {Z, Q}, {Z, Z}};
    for (auto &pr : pairs) {
        bool oka, okb;
        const G a = rd(pr[0], oka), b = rd(pr[1], okb);
        if (!oka || !okb) abort();
        put(g, "add_a", enc(pr[0]));
        put(g, "add_b", enc(pr[1]));
        put(g, "add_out", enc(a + b));
    }
    const Fr muls[4] = {Fr(7).inverse(), Fr::zero(), Fr::one(), -Fr::one()};
    for (auto &s : muls) {
        const G p = rd(bases[5], ok);
        put(g, "mul_p", enc(bases[5]));
        put(g, "mul_s", enc_f(s));
        put(g, "mul_out", enc(s * p));
    }

    // curve points by square root: x = 2, 3, ... until y^2 = x^3 + a x + b has a solution
    std::vector<G> found;
    for (long k = 2; found.size() < 6; ++k) {
        Fc x = Fc::one();
        for (long j = 1; j < k; ++j) x = x + Fc::one();
        if (with_cofactor) x = x + x.squared() * G::coeff_b;   // an x with both Fq2 components set
        const Fc rhs = x.squared() * x + G::coeff_a * x + G::coeff_b;
        if ((rhs ^ Fc::euler) != Fc::one()) continue;
        G p;
        p.X = x;
        p.Y = rhs.sqrt();
        p.Z = Fc::one();
        if (!p.is_well_formed()) abort();
        found.push_back(p);
    }
    if (with_cofactor) {
        const size_t m = found.size();
        for (size_t i = 0; i < m; ++i) found.push_back(G::h * found[i]);
    }
    for (auto &p : found) {
        rd(p, ok);
        put(g, "curve_points", enc(p));
        put(g, "curve_points_ok", std::vector<unsigned char>(1, ok ? 1 : 0));
    }
}

int main()
{
    inhibit_profiling_info = true;
    inhibit_profiling_counters = true;
    mnt4_pp::init_public_params();
    mnt6_pp::init_public_params();
    emit<mnt4_G1, mnt4_Fr, mnt4_Fq>("mnt4_g1", false);
    emit<mnt4_G2, mnt4_Fr, mnt4_Fq2>("mnt4_g2", true);
    emit<mnt6_G1, mnt6_Fr, mnt6_Fq>("mnt6_g1", false);
    return 0;
}
"""


def run_driver():
    if not os.path.isdir(os.path.join(REF, "libff")):
        sys.exit(f"the reference is not mounted at {REF}")
    if not os.path.isdir(GMPINC):
        subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    srcs = []
    for sub in ("libff/algebra/curves/mnt/mnt4", "libff/algebra/curves/mnt/mnt6", "libff/algebra/curves/mnt"):
        d = os.path.join(REF, sub)
        srcs += [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".cpp")]
    srcs += [os.path.join(REF, "libff", p) for p in ("common/profiling.cpp", "common/utils.cpp", "common/double.cpp",
                                                     "algebra/serialization.cpp")]
    gmplib = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"
    flags = ["-std=c++11", "-O2", "-DNDEBUG", "-DCURVE_ALT_BN128", "-DNO_PROCPS", "-DBINARY_OUTPUT", "-DMONTGOMERY_OUTPUT",
             "-DUSE_ASM", "-w", "-I" + REF, "-I" + GMPINC]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ffi_mnt_driver.cpp"), os.path.join(d, "ffi_mnt_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        objs = []
        procs = []
        for i, s in enumerate([src] + srcs):
            o = os.path.join(d, f"o{i}.o")
            objs.append(o)
            procs.append(subprocess.Popen(["g++", *flags, "-c", s, "-o", o]))
        for p in procs:
            if p.wait() != 0:
                sys.exit("compiling the driver failed")
        subprocess.check_call(["g++", "-o", exe, *objs, gmplib if os.path.exists(gmplib) else "-lgmp", "-lcrypto",
                               "-lpthread"])
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def main():
    rows = {}
    for line in run_driver().splitlines():
        if "/" not in line or " " not in line:
            continue
        key, hx = line.split(" ", 1)
        rows.setdefault(key, []).append(np.frombuffer(bytes.fromhex(hx.strip()), dtype=np.uint8))
    out = {}
    for key, vals in rows.items():
        a = np.stack(vals)
        if key.endswith("/msm_out"):
            a = a[0]
        elif key.endswith("_ok"):
            a = a.reshape(-1)
        out[key] = a
    for g in ("mnt4_g1", "mnt4_g2", "mnt6_g1"):
        ok = out[f"{g}/curve_points_ok"]
        assert out[f"{g}/bases"].shape[0] == 64 and int(ok.sum()) >= 4, g
        print(g, {k.split("/")[1]: v.shape for k, v in out.items() if k.startswith(g + "/")}, "ok:", ok.tolist())
    ok = out["mnt4_g2/curve_points_ok"]
    assert int((ok == 0).sum()) >= 4 and int((ok == 1).sum()) >= 4, "mnt4_g2: 4 rejected and 4 accepted twist points"
    path = os.path.join(HERE, "ffi_mnt.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
