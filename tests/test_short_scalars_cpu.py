"""amdmsm_*_short without a device: the symbols and the descriptor's layout, amdmsm_plan_short against the closed form
and against amdmsm_plan_ex at full width, the split rule, the bound on the chosen window size, and -- on a model of the
signed recoding -- that (bits + 2 + c - 1) / c windows hold every scalar below 2^bits without a carry out."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "amdmsm.h")
NEW_SYMBOLS = ["amdmsm_plan_short", "amdmsm_scalar_bits_device", "amdmsm_multi_exp_short", "amdmsm_msm_device_short"]
# (curve, group) of the eleven groups
ALL_GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1)]
BITS = [1, 2, 7, 8, 14, 15, 16, 30, 31, 32, 33, 62, 63, 64, 127, 128]
FORCED_C = [4, 8, 13, 16]
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return ctypes.CDLL(libff_amd.engine.SO_PATH)


def plan_short(lib, curve, group, n, bits, window_bits=0, endomorphism=0):
    assert hasattr(lib, "amdmsm_plan_short"), "amdmsm_plan_short is not exported by libamdmsm.so"
    c, w, used, b, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_uint32(0), ctypes.c_size_t(0)
    rc = lib.amdmsm_plan_short(curve, group, ctypes.c_size_t(n), window_bits, endomorphism, bits, ctypes.byref(c),
                               ctypes.byref(w), ctypes.byref(b), ctypes.byref(ws), ctypes.byref(used))
    return rc, (c.value, w.value, b.value, ws.value, used.value)


def plan_ex(lib, curve, group, n, window_bits=0, endomorphism=0):
    c, w, used, b, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_uint32(0), ctypes.c_size_t(0)
    rc = lib.amdmsm_plan_ex(curve, group, ctypes.c_size_t(n), window_bits, endomorphism, ctypes.byref(c), ctypes.byref(w),
                            ctypes.byref(b), ctypes.byref(ws), ctypes.byref(used))
    return rc, (c.value, w.value, b.value, ws.value, used.value)


def fr_bits(lib, curve, group):
    out = (ctypes.c_size_t * 4)()
    assert lib.amdmsm_sizes(curve, group, out) == 0
    return int(out[3])


def split_bound_x1000(lib, curve, group):
    """ceil(1000 log2) of the split's bound on |k1|, |k2|; None where the group has no endomorphism"""
    out = (ctypes.c_size_t * 4)()
    assert lib.amdmsm_sizes(curve, group, out) == 0
    lam = (ctypes.c_uint8 * int(out[0]))()
    bound, prime = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.amdmsm_endomorphism_info(curve, group, lam, ctypes.byref(bound), ctypes.byref(prime))
    return bound.value if rc == 0 else None


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_symbol_is_exported_and_declared(lib, symbol):
    assert hasattr(lib, symbol), f"{symbol} is not exported by libamdmsm.so"
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % symbol, text), f"{symbol} is not declared in amdmsm.h"
    import libff_amd.engine as e

    assert symbol in e.EXPORTED_SYMBOLS


def test_scalar_desc_layout_matches_the_header(lib, tmp_path):
    """sizeof, AMDMSM_SCALAR_DESC_INIT, every field offset and the kind values, as a C probe compiled against the header
    prints them; the ABI version did not move."""
    import libff_amd.engine as e

    assert hasattr(e, "ScalarDesc"), "libff_amd.engine has no mirror of amdmsm_scalar_desc"
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = [f[0] for f in e.ScalarDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "amdmsm.h"\nint main(void) {\n'
                   '    amdmsm_scalar_desc d = AMDMSM_SCALAR_DESC_INIT;\n'
                   '    printf("%zu %u %d %d", sizeof(amdmsm_scalar_desc), d.struct_size, d.kind, d.bits);\n' +
                   "".join('    printf(" %%zu", offsetof(amdmsm_scalar_desc, %s));\n' % f for f in fields) +
                   '    printf(" %d %d %d %d %d %d", AMDMSM_SCALAR_FR, AMDMSM_SCALAR_U8, AMDMSM_SCALAR_U16, AMDMSM_SCALAR_U32,'
                   ' AMDMSM_SCALAR_U64, AMDMSM_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == got[1] == ctypes.sizeof(e.ScalarDesc)
    assert got[2:4] == [0, 0]   # the initialiser leaves kind = Fr records and bits = full width
    nf = len(fields)
    assert got[4:4 + nf] == [getattr(e.ScalarDesc, f).offset for f in fields]
    assert got[4 + nf:] == [e.SCALAR_FR, e.SCALAR_U8, e.SCALAR_U16, e.SCALAR_U32, e.SCALAR_U64, 3] == [0, 1, 2, 4, 8, 3]
    assert lib.amdmsm_abi_version() == 3


def test_public_names(lib):
    import libff_amd

    for name in ("multi_exp_short", "msm_device_short", "scalar_bits"):
        assert hasattr(libff_amd.Engine, name), name
    assert hasattr(libff_amd, "plan_short")
    p = libff_amd.plan_short(0, 1, 1 << 16, 32, window_bits=8)
    assert (p["c"], p["num_windows"], p["endomorphism"]) == (8, 5, False)


@pytest.mark.parametrize("curve,group", [(0, 1), (1, 2), (4, 1)])
def test_window_count_is_the_closed_form(lib, curve, group):
    fb = fr_bits(lib, curve, group)
    for bits in BITS + [fb]:
        for c in FORCED_C:
            for endo in (-1, 0):
                rc, (c_out, w, b, ws, used) = plan_short(lib, curve, group, 1 << 16, bits, c, endo)
                assert rc == 0, (bits, c)
                if used:   # only above the split's bound, and then it is the ordinary plan
                    assert bits * 1000 > split_bound_x1000(lib, curve, group)
                    assert (c_out, w, b, ws, used) == plan_ex(lib, curve, group, 1 << 16, c, endo)[1]
                    continue
                assert c_out == c and b == 1 << (c - 1)
                assert w == (bits + 2 + c - 1) // c, (bits, c, w)
                assert ws > 0


@pytest.mark.parametrize("curve,group", ALL_GROUPS)
def test_full_width_is_the_ordinary_plan(lib, curve, group):
    fb = fr_bits(lib, curve, group)
    for n in (1 << 10, 1 << 16, 1 << 20):
        for endo in (0, 1, -1):
            want = plan_ex(lib, curve, group, n, 0, endo)
            assert want[0] == 0
            assert plan_short(lib, curve, group, n, fb, 0, endo) == want, (n, endo)
            assert plan_short(lib, curve, group, n, 0, 0, endo) == want, (n, endo)   # 0 = full width


@pytest.mark.parametrize("curve,group", ALL_GROUPS)
def test_no_split_at_or_below_its_bound(lib, curve, group):
    bound = split_bound_x1000(lib, curve, group)
    fb = fr_bits(lib, curve, group)
    top = fb - 1 if bound is None else bound // 1000   # floor: the largest whole bit count not above the bound
    for n in (1 << 10, 1 << 16, 1 << 20):
        for bits in [b for b in BITS if b <= top] + [top]:
            for endo in (0, 1, 2):
                for c in (0, 13):
                    rc, (c_out, w, b, ws, used) = plan_short(lib, curve, group, n, bits, c, endo)
                    assert rc == 0 and used == 0, (n, bits, endo, c)
                    assert w == (bits + 2 + c_out - 1) // c_out


@pytest.mark.parametrize("curve,group", ALL_GROUPS)
def test_chosen_window_is_at_most_bits_plus_two(lib, curve, group):
    for n in (1, 1000, 1 << 10, 1 << 16, 1 << 20, 1 << 24):
        for bits in BITS:
            rc, (c, w, b, ws, used) = plan_short(lib, curve, group, n, bits, 0, -1)
            assert rc == 0
            assert 2 <= c <= min(bits + 2, 22), (n, bits, c)
            assert w == (bits + 2 + c - 1) // c and b == 1 << (c - 1)


def test_refusals(lib):
    assert plan_short(lib, 0, 1, 1000, 32, 23)[0] == BAD_ARG      # window_bits > 22, as for the batch calls
    assert plan_short(lib, 0, 1, 1000, -1)[0] == BAD_ARG          # a plan needs a bit length
    assert plan_short(lib, 5, 2, 1000, 32)[0] == -3               # (MNT6, G2)


def signed_digits(k, c, num_windows):
    """field_get_signed_digits (field_utils.tcc:205-239) as the device recodes it: digit = raw + carry; 2^c -> 0 with a
    carry; bit c - 1 set -> digit - 2^c with a carry.  Returns the digits and the carry left after the last window."""
    digits, carry = [], 0
    for w in range(num_windows):
        d = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        if d >> c:
            d, carry = 0, 1
        elif (d >> (c - 1)) & 1:
            d, carry = d - (1 << c), 1
        else:
            carry = 0
        digits.append(d)
    return digits, carry


def test_recoding_model_agrees_with_the_test_suite_model():
    """the model above against the one the tail tests use, so that the property below is about the same recoding"""
    import tail_cases

    other = tail_cases.signed_digits
    for k in (0, 1, 255, 256, (1 << 64) - 1, 0x8000, 0x123456789abcdef):
        for c in (4, 13, 16):
            W = (64 + 2 + c - 1) // c
            assert list(other(k, c, W)) == signed_digits(k, c, W)[0]


@pytest.mark.parametrize("c", FORCED_C + [2, 3, 5, 10, 22])
def test_short_window_count_holds_every_scalar_without_a_carry_out(lib, c):
    """2^bits - 1 (all ones: the carry runs through every window) and 2^(bits - 1) reconstruct from num_windows digits,
    every digit within the bucket range, no carry left: the property the "+ 2" exists for"""
    for bits in BITS + [254, 298]:
        rc, (c_out, W, b, ws, used) = plan_short(lib, 4, 1, 1 << 12, bits, c, -1)   # MNT4: Fr has 298 bits
        assert rc == 0 and c_out == c and W == (bits + 2 + c - 1) // c
        for k in {(1 << bits) - 1, 1 << (bits - 1), ((1 << bits) - 1) // 3, 1, 0}:
            digits, carry = signed_digits(k, c, W)
            assert carry == 0, (bits, c, k)
            assert all(-(1 << (c - 1)) <= d < (1 << (c - 1)) for d in digits)
            assert sum(d << (c * w) for w, d in enumerate(digits)) == k
