"""The template shim routes the MNT groups: a translation unit that includes mnt4_pp.hpp, mnt6_pp.hpp and
libff_amd/multiexp.hpp and calls libff::multi_exp for mnt4_G1, mnt4_G2 and mnt6_G1 references the engine's
amdmsm_multi_exp; for mnt6_G2 (Fq3, no device implementation) it does not.  CPU only; needs the reference headers and
the gmp.h that the reference build (oracle/build_ref.sh) stages, otherwise skipped."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LIBFF_REFERENCE", "/root/reference")   # as oracle/build_ref.sh
GMPINC = os.path.join(ROOT, "oracle", "_ref", "gmpinc")

SRC = r"""
#include <libff/algebra/curves/mnt/mnt4/mnt4_pp.hpp>
#include <libff/algebra/curves/mnt/mnt6/mnt6_pp.hpp>
#include <libff_amd/multiexp.hpp>
GROUP_T run(const std::vector<GROUP_T> &b, const std::vector<FIELD_T> &s)
{
    return libff::multi_exp<GROUP_T, FIELD_T, libff::multi_exp_method_BDLO12_signed, libff::multi_exp_base_form_normal>(
        b.cbegin(), b.cend(), s.cbegin(), s.cend(), 1);
}
"""


@pytest.mark.parametrize("group,field,routed", [("mnt4_G1", "mnt4_Fr", True), ("mnt4_G2", "mnt4_Fr", True),
                                                ("mnt6_G1", "mnt6_Fr", True), ("mnt6_G2", "mnt6_Fr", False)])
def test_shim_routes_mnt_groups(group, field, routed):
    if not os.path.isdir(os.path.join(REF, "libff")) or not os.path.isdir(GMPINC):
        pytest.skip("reference headers not available here")
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "route.cpp"), os.path.join(d, "route.o")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = ["g++", "-std=c++11", "-O0", "-c", "-DNDEBUG", "-DCURVE_ALT_BN128", "-DNO_PROCPS", "-DBINARY_OUTPUT",
               "-DMONTGOMERY_OUTPUT", "-DUSE_ASM", "-w", f"-DGROUP_T=libff::{group}", f"-DFIELD_T=libff::{field}",
               "-I" + REF, "-I" + GMPINC, "-I" + os.path.join(ROOT, "include"), src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        undef = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.split()
    assert ("amdmsm_multi_exp" in undef) == routed, group
