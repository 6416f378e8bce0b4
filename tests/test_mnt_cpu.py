"""MNT4-298 / MNT6-298 G1 on the host side of the C ABI (no device): record sizes as libff lays them out (bigint<5>
coordinates and scalars), the planner for 298-bit scalars, the endomorphism reported unused whatever is asked,
the G2 groups refused; and the pure-integer model the GPU tests check against."""
import ctypes

import pytest

import mnt_model as mm

import libff_amd
from libff_amd import G1, G2, MNT4, MNT6


GROUPS = [(MNT4, G1), (MNT4, G2), (MNT6, G1)]


@pytest.mark.parametrize("curve,group", GROUPS)
def test_sizes_match_libff(curve, group):
    # sizeof(mnt4_G1) = sizeof(mnt6_G1) = 120 (three bigint<5>), sizeof(mnt4_G2) = 240, sizeof(Fr) = 40, 298-bit Fr
    k = 1 if group == G1 else 2
    assert libff_amd.sizes(curve, group) == {"fr_bytes": 40, "g_bytes": 120 * k, "affine_bytes": 80 * k, "fr_bits": 298}


@pytest.mark.parametrize("curve,group", GROUPS)
def test_plan_has_no_endomorphism(curve, group):
    for n in (1, 257, 1 << 16, 1 << 20, 1 << 22):
        for e in (-1, 0, 1, 2):
            p = libff_amd.plan(curve, group, n, endomorphism=e)
            assert p["endomorphism"] is False
            assert p["num_windows"] == (298 + 2 + p["c"] - 1) // p["c"]
    for c in (2, 3, 5, 8, 13, 16, 20):
        assert libff_amd.plan(curve, group, 1 << 16, window_bits=c)["c"] == c
    with pytest.raises(libff_amd.AmdMsmError):
        libff_amd.endomorphism_info(curve, group)


def test_mnt6_g2_refused():
    lib = libff_amd.load_library()
    out = (ctypes.c_size_t * 4)()
    assert lib.amdmsm_sizes(MNT6, G2, out) == -3   # AMDMSM_ERR_UNSUPPORTED
    assert libff_amd.engine.CURVE_NAMES[MNT4] == "mnt4" and libff_amd.engine.CURVE_NAMES[MNT6] == "mnt6"


@pytest.mark.parametrize("model", [mm.MNT4, mm.MNT4_G2, mm.MNT6], ids=["mnt4_g1", "mnt4_g2", "mnt6_g1"])
def test_model(model):
    # the cycle: each curve's group order is the other's field
    other = mm.MNT6 if model.p == mm.MNT4.p else mm.MNT4
    assert model.r == other.p and model.a in (2, 11, (34, 0))
    assert model.mul(model.r, model.one) is mm.INF
    P = model.mul(12345, model.one)
    assert model.add(P, model.neg(P)) is mm.INF
    assert model.dbl(P) == model.mul(2 * 12345, model.one)
    assert model.point(model.records([P], [77])[0]) == P
    assert model.point(model.records([mm.INF])[0]) is mm.INF
