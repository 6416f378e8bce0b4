"""Radix-2 FFT over a point vector (amdmsm_group_fft / _device / amdmsm_plan_group_fft / amdmsm_fr_modulus) as far as a
host without a GPU can see it: the symbols are exported and declared, the Python engine has the methods, (MNT6, G2) is
refused, the plan counts stages and sizes chunks by the 1 GiB rule, and fft_twiddles makes powers of a root of unity."""
import ctypes
import inspect
import os

import pytest

import mnt_model as mm
from common import golden, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_group_fft", "amdmsm_group_fft_device", "amdmsm_plan_group_fft", "amdmsm_fr_modulus")
BAD_ARG, UNSUPPORTED, TOO_LARGE = -2, -3, -5
PAIRING = [(c, g) for c in (0, 1, 2, 3) for g in (1, 2)]   # alt_bn128, bls12_377, bw6_761, bls12_381: G1, G2
MNT = [(4, 1), (4, 2), (5, 1)]
CURVE_NAMES = {0: "alt_bn128", 1: "bls12_377", 2: "bw6_761", 3: "bls12_381"}
TWO_ADICITY = {0: 28, 1: 47, 2: 46, 3: 32, 4: 34, 5: 17}


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def test_the_symbols_are_exported_and_declared(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header
    assert "#define AMDMSM_ABI_VERSION 3" in header


def test_engine_has_the_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.group_fft).parameters
    assert list(host)[:5] == ["self", "curve", "group", "points", "twiddles"]
    assert list(host)[5:9] == ["base_form", "out_form", "scalars_plain", "chunk_points"]
    assert host["out_form"].default == libff_amd.OUT_LIBFF and host["scalars_plain"].default is False
    assert host["chunk_points"].default == 0 and host["base_form"].default == libff_amd.multi_exp_base_form_normal
    dev = inspect.signature(libff_amd.Engine.group_fft_device).parameters
    assert list(dev)[:7] == ["self", "curve", "group", "d_points", "n", "d_twiddles", "d_out_xyz"]
    assert list(dev)[7:] == ["out_form", "scalars_plain", "chunk_points", "stream"]
    assert dev["out_form"].default == libff_amd.OUT_LIBFF and dev["scalars_plain"].default is False
    assert dev["chunk_points"].default == 0 and dev["stream"].default is None
    for name in ("plan_group_fft", "fr_modulus", "fft_twiddles"):
        assert name in libff_amd.__all__ and callable(getattr(libff_amd, name)), name
    plan = inspect.signature(libff_amd.plan_group_fft).parameters
    assert list(plan) == ["curve", "group", "n", "chunk_points"] and plan["chunk_points"].default == 0
    tw = inspect.signature(libff_amd.fft_twiddles).parameters
    assert list(tw) == ["curve", "n", "inverse"] and tw["inverse"].default is False


def test_mnt6_g2_is_refused(lib):
    """the group the library does not carry is refused before the context is looked at; a group it carries asks for one"""
    from libff_amd import G1, G2, MNT6

    z = ctypes.c_size_t(0)
    host = lambda group: lib.amdmsm_group_fft(None, MNT6, group, None, z, 0, z, None, None, z, None)
    dev = lambda group: lib.amdmsm_group_fft_device(None, MNT6, group, None, z, None, None, z, None)
    assert host(G2) == UNSUPPORTED and dev(G2) == UNSUPPORTED
    assert host(G1) == BAD_ARG and dev(G1) == BAD_ARG
    out = (ctypes.c_size_t * 6)()
    assert lib.amdmsm_plan_group_fft(MNT6, G2, ctypes.c_size_t(8), z, out) == UNSUPPORTED
    assert lib.amdmsm_plan_group_fft(MNT6, G1, ctypes.c_size_t(8), z, out) == 0
    assert lib.amdmsm_plan_group_fft(MNT6, G1, ctypes.c_size_t(8), z, None) == BAD_ARG
    assert lib.amdmsm_fr_modulus(MNT6, G2, (ctypes.c_uint8 * 40)()) == UNSUPPORTED


@pytest.mark.parametrize("curve,group", PAIRING + MNT)
def test_plan_counts_stages(lib, curve, group):
    from libff_amd import plan_group_fft

    for n, stages in ((1, 0), (2, 1), (4, 2), (1024, 10), (1 << 20, 20)):
        p = plan_group_fft(curve, group, n)
        assert p["stages"] == stages
        assert p["ladder_stages"] == max(stages - 1, 0)   # the stage whose twiddles are all 1 has no ladder
        assert p["scalar_muls"] == n // 2 * max(stages - 1, 0)
        assert p["chunk_points"] == min(n // 2, plan_group_fft(curve, group, 1 << 28)["chunk_points"])
        assert p["chunk_bytes"] <= p["workspace_bytes"]


@pytest.mark.parametrize("curve,group", PAIRING + MNT)
def test_plan_chunks(lib, curve, group):
    from libff_amd import plan_group_fft, sizes

    s = sizes(curve, group)
    aff = s["affine_bytes"]
    p = plan_group_fft(curve, group, 1 << 28)
    cn = p["chunk_points"]
    assert cn % 256 == 0 and cn >= 256
    assert p["chunk_bytes"] <= 1 << 30
    assert p["chunk_bytes"] >= 16 * aff * cn                      # smv_table's records and scratch, at the least
    assert p["chunk_bytes"] // cn * (cn + 256) > 1 << 30          # 256 butterflies more would not fit
    assert p["chunk_bytes"] % cn == 0
    # the rest is linear in n: two vectors of compact affine records and one of libff records
    assert p["workspace_bytes"] - p["chunk_bytes"] >= (1 << 28) * (2 * aff + s["g_bytes"])
    assert p["workspace_bytes"] - p["chunk_bytes"] < (1 << 28) * (2 * aff + s["g_bytes"]) + 4096
    # never more than there is; a caller's value is taken as given
    assert plan_group_fft(curve, group, 128)["chunk_points"] == 64
    assert plan_group_fft(curve, group, 1024, chunk_points=64)["chunk_points"] == 64
    assert plan_group_fft(curve, group, 1024, chunk_points=192)["chunk_points"] == 192
    assert plan_group_fft(curve, group, 16, chunk_points=64)["chunk_points"] == 8
    assert plan_group_fft(curve, group, 1 << 28, chunk_points=100)["chunk_points"] == 100


@pytest.mark.parametrize("curve,group", PAIRING + MNT)
def test_plan_refuses_bad_sizes(lib, curve, group):
    out = (ctypes.c_size_t * 6)()
    z = ctypes.c_size_t(0)
    for n in (3, 6, 1025):
        assert lib.amdmsm_plan_group_fft(curve, group, ctypes.c_size_t(n), z, out) == BAD_ARG
    assert lib.amdmsm_plan_group_fft(curve, group, ctypes.c_size_t(1 << 29), z, out) == TOO_LARGE
    assert lib.amdmsm_plan_group_fft(curve, group, ctypes.c_size_t(1 << 28), z, out) == 0


@pytest.mark.parametrize("curve,group", PAIRING + MNT)
def test_fr_modulus(lib, curve, group):
    from libff_amd import fr_modulus

    if curve in CURVE_NAMES:
        want = to_int(golden()[f"{CURVE_NAMES[curve]}_g1/fr_modulus"])
    else:
        want = {4: mm.MNT4, 5: mm.MNT6}[curve].r
    assert fr_modulus(curve, group) == want


@pytest.mark.parametrize("curve", sorted(TWO_ADICITY))
def test_fft_twiddles(lib, curve):
    from libff_amd import fft_twiddles, fr_modulus, sizes

    r = fr_modulus(curve, 1)
    limbs = sizes(curve, 1)["fr_bytes"] // 8
    s = TWO_ADICITY[curve]
    assert (r - 1) % (1 << s) == 0 and (r - 1) % (1 << (s + 1)) != 0
    for n in (2, 4, 8, 1024, 1 << 17):
        fwd, inv = fft_twiddles(curve, n), fft_twiddles(curve, n, inverse=True)
        assert fwd.shape == inv.shape == (n // 2, limbs) and fwd.dtype == inv.dtype == "uint64"
        f, i = [to_int(row) for row in fwd], [to_int(row) for row in inv]
        assert f[0] == 1 and i[0] == 1
        w = f[1] if n > 2 else r - 1
        assert pow(w, n // 2, r) == r - 1                       # a primitive n-th root
        step = max(1, n // 2 // 64)
        assert all(f[k] == pow(w, k, r) for k in range(0, n // 2, step))
        assert all(a * b % r == 1 for a, b in zip(f, i))
    assert fft_twiddles(curve, 1).shape == (0, limbs)
    with pytest.raises(ValueError):
        fft_twiddles(curve, 1 << (s + 1))
    with pytest.raises(ValueError):
        fft_twiddles(curve, 12)


def test_fft_twiddles_mnt6_stops_at_its_two_adicity(lib):
    from libff_amd import MNT6, fft_twiddles

    with pytest.raises(ValueError):
        fft_twiddles(MNT6, 1 << 18)
