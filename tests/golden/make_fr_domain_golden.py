#!/usr/bin/env python3
"""Generate tests/golden/fr_domain.npz: what the reference says about the radix-2 domains of the six scalar fields.

Runs ONLY where the reference is mounted (LIBFF_REFERENCE, default /root/reference): the driver below is compiled
against the reference's curve sources, in a temporary directory, with the flags of oracle/build_ref.sh.  The file holds
data only.  Per scalar field <c> in alt_bn128, bls12_377, bw6_761, bls12_381, mnt4, mnt6, as plain little-endian 64-bit
words (as_bigint):

  <c>/s                         Fr::s, the 2-adicity of r - 1
  <c>/root_of_unity             Fr::root_of_unity
  <c>/multiplicative_generator  Fr::multiplicative_generator
  <c>/root_1, root_4, root_s    get_root_of_unity<Fr>(2^k) for k = 1, 4, s   (libff/algebra/fields/field_utils.tcc)

has_root_of_unity compares n with 1u << logn, a 32-bit shift, so the reference's get_root_of_unity throws for every
n >= 2^32 -- which is k = s for all fields but alt_bn128 (s = 28) and mnt6 (s = 17).  There root_s is Fr::root_of_unity
itself, which is what the 2^s-th root is.  The file is about 8 KB: a few hundred bytes of words under npz's per-array
headers.
"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LIBFF_REFERENCE", "/root/reference")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <libff/algebra/curves/alt_bn128/alt_bn128_pp.hpp>
#include <libff/algebra/curves/bls12_377/bls12_377_pp.hpp>
#include <libff/algebra/curves/bw6_761/bw6_761_pp.hpp>
#include <libff/algebra/curves/bls12_381/bls12_381_pp.hpp>
#include <libff/algebra/curves/mnt/mnt4/mnt4_pp.hpp>
#include <libff/algebra/curves/mnt/mnt6/mnt6_pp.hpp>
#include <libff/algebra/fields/field_utils.hpp>
#include <libff/common/profiling.hpp>

using namespace libff;

template<typename Fr> static void put(const char *c, const char *key, const Fr &x)
{
    const auto b = x.as_bigint();
    printf("%s/%s", c, key);
    for (size_t i = 0; i < sizeof(b.data) / sizeof(b.data[0]); ++i) printf(" %016lx", (unsigned long)b.data[i]);
    printf("\n");
}
template<typename Fr> static Fr root(size_t logn)
{
    try {
        return get_root_of_unity<Fr>((size_t)1 << logn);
    } catch (const std::invalid_argument &) {
        if (logn < 32 || logn != Fr::s) abort();   // only the 32-bit shift of has_root_of_unity, and only at k = s
        return Fr::root_of_unity;                  // the 2^s-th root is the field's constant itself
    }
}
template<typename Fr> static void emit(const char *c)
{
    printf("%s/s %016lx\n", c, (unsigned long)Fr::s);
    put(c, "root_of_unity", Fr::root_of_unity);
    put(c, "multiplicative_generator", Fr::multiplicative_generator);
    put(c, "root_1", root<Fr>(1));
    put(c, "root_4", root<Fr>(4));
    put(c, "root_s", root<Fr>(Fr::s));
}

int main()
{
    inhibit_profiling_info = true;
    inhibit_profiling_counters = true;
    alt_bn128_pp::init_public_params();
    bls12_377_pp::init_public_params();
    bw6_761_pp::init_public_params();
    bls12_381_pp::init_public_params();
    mnt4_pp::init_public_params();
    mnt6_pp::init_public_params();
    emit<alt_bn128_Fr>("alt_bn128");
    emit<bls12_377_Fr>("bls12_377");
    emit<bw6_761_Fr>("bw6_761");
    emit<bls12_381_Fr>("bls12_381");
    emit<mnt4_Fr>("mnt4");
    emit<mnt6_Fr>("mnt6");
    return 0;
}
"""


def run_driver():
    if not os.path.isdir(os.path.join(REF, "libff")):
        sys.exit(f"the reference is not mounted at {REF}")
    srcs = []
    for sub in ("alt_bn128", "bls12_377", "bw6_761", "bls12_381", "mnt/mnt4", "mnt/mnt6", "mnt"):
        srcs += sorted(glob.glob(os.path.join(REF, "libff/algebra/curves", sub, "*.cpp")))
    srcs += [os.path.join(REF, "libff", p) for p in ("common/profiling.cpp", "common/utils.cpp", "common/double.cpp",
                                                     "algebra/serialization.cpp")]
    gmplib = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"
    with tempfile.TemporaryDirectory() as d:
        # gmp.h alone, as oracle/build_ref.sh stages it
        gmph = next(c for c in ("/usr/include/gmp.h", "/usr/include/x86_64-linux-gnu/gmp.h", "/opt/conda/include/gmp.h")
                    if os.path.exists(c))
        os.makedirs(os.path.join(d, "gmpinc"))
        shutil.copy(gmph, os.path.join(d, "gmpinc", "gmp.h"))
        flags = ["-std=c++11", "-O1", "-DNDEBUG", "-DCURVE_ALT_BN128", "-DNO_PROCPS", "-DBINARY_OUTPUT", "-DMONTGOMERY_OUTPUT",
                 "-DUSE_ASM", "-w", "-I" + REF, "-I" + os.path.join(d, "gmpinc")]
        src, exe = os.path.join(d, "fr_domain_driver.cpp"), os.path.join(d, "fr_domain_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        objs, procs = [], []
        for i, s in enumerate([src] + srcs):
            o = os.path.join(d, f"o{i}.o")
            objs.append(o)
            procs.append(subprocess.Popen(["g++", *flags, "-c", s, "-o", o]))
        for p in procs:
            if p.wait() != 0:
                sys.exit("compiling the driver failed")
        subprocess.check_call(["g++", "-o", exe, *objs, gmplib if os.path.exists(gmplib) else "-lgmp", "-lcrypto", "-lpthread"])
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def main():
    out = {}
    for line in run_driver().splitlines():
        if "/" not in line or " " not in line:
            continue
        key, *words = line.split()
        out[key] = np.array([int(w, 16) for w in words], dtype=np.uint64)
    for c in ("alt_bn128", "bls12_377", "bw6_761", "bls12_381", "mnt4", "mnt6"):
        assert {k.split("/")[1] for k in out if k.startswith(c + "/")} == {
            "s", "root_of_unity", "multiplicative_generator", "root_1", "root_4", "root_s"}, c
        print(c, "s =", int(out[c + "/s"][0]), "generator =", int(out[c + "/multiplicative_generator"][0]))
    path = os.path.join(HERE, "fr_domain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
