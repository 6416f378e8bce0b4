"""The FFI surface for bls12_381, MNT4-298 and MNT6-298 and the loaded-bases calls, as far as a host without a GPU can
check it: the names are declared and exported, the wire sizes are the reference's, and the MNT fixtures of
tests/golden/ffi_mnt.npz (recorded from the reference's own codecs, multi_exp and group law by
tests/golden/make_ffi_mnt_golden.py) agree with the integer model of tests/mnt_model.py -- which is what lets the GPU
tests use that model for the cases the fixture does not hold."""
import ctypes
import os
import re

import numpy as np
import pytest

import ffi_wire as fw
import mnt_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libff_amd_ffi.h")

NEW_SYMBOLS = (
    [f"{g}_multiexp" for g in ("bls12_381_g1", "bls12_381_g2", "mnt4_g1", "mnt4_g2", "mnt6_g1")]
    + [f"{c}_{op}" for c in ("bls12_381", "mnt4", "mnt6") for op in ("init", "g1_add", "g1_mul")]
    + ["amdmsm_ffi_bases_load", "amdmsm_ffi_multiexp_loaded", "amdmsm_ffi_bases_free"])


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return ctypes.CDLL(libff_amd.engine.SO_PATH)


def test_new_names_are_declared_and_exported(lib):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b([a-z][a-z0-9_]+)\s*\(", text))
    assert len(NEW_SYMBOLS) == 17
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in libff_amd_ffi.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # MNT6 G2 stays out
    assert "mnt6_g2_multiexp" not in declared and not hasattr(lib, "mnt6_g2_multiexp")


def test_element_sizes(lib):
    import libff_amd

    assert libff_amd.ffi is not None
    es = libff_amd.ffi.element_sizes
    assert es(libff_amd.BLS12_381, 1) == {"fr_bytes": 32, "element_bytes": 96}
    assert es(libff_amd.BLS12_381, 2) == {"fr_bytes": 32, "element_bytes": 192}
    assert es(libff_amd.MNT4, 1) == {"fr_bytes": 40, "element_bytes": 80}
    assert es(libff_amd.MNT4, 2) == {"fr_bytes": 40, "element_bytes": 160}
    assert es(libff_amd.MNT6, 1) == {"fr_bytes": 40, "element_bytes": 80}
    assert es("mnt4", 2) == es(libff_amd.MNT4, 2)
    with pytest.raises(libff_amd.AmdMsmError):
        es(libff_amd.MNT6, 2)
    assert len(libff_amd.ffi.GROUPS) == 11
    for name, (C, curve, group) in fw.MNT_GROUPS.items():
        assert es(curve, group)["element_bytes"] == fw.element_bytes(C)
        assert libff_amd.ffi.symbol_name(curve, group) == f"{name}_multiexp"


@pytest.mark.parametrize("name", sorted(fw.MNT_GROUPS))
def test_fixture_points_are_on_the_model_curve(name):
    C = fw.MNT_GROUPS[name][0]
    f = fw.fixtures()
    E = fw.element_bytes(C)
    for key in ("bases", "add_a", "add_b", "add_out", "mul_p", "mul_out", "curve_points"):
        rows = f[f"{name}/{key}"]
        assert rows.shape[1] == E and rows.dtype == np.uint8, key
        for k in range(rows.shape[0]):
            assert C.on_curve(fw.decode_point(C, rows[k])), (key, k)
    assert f[f"{name}/bases"].shape == (64, E) and f[f"{name}/scalars"].shape == (64, fw.FB)
    assert C.on_curve(fw.decode_point(C, f[f"{name}/msm_out"]))
    for k in range(64):
        assert fw.decode_scalar(f[f"{name}/scalars"][k]) < C.r
        assert fw.decode_point(C, f[f"{name}/bases"][k]) == C.mul(17 + k, C.one)   # bases are (17 + k) G


@pytest.mark.parametrize("name", sorted(fw.MNT_GROUPS))
def test_subgroup_verdicts_are_the_reference_flags(name):
    """[r]P == 0 in the model is what the reference's group_element_read returned for every fixture point."""
    C = fw.MNT_GROUPS[name][0]
    f = fw.fixtures()
    pts, ok = f[f"{name}/curve_points"], f[f"{name}/curve_points_ok"]
    assert pts.shape[0] == ok.shape[0] and int(ok.sum()) >= 4
    for k in range(pts.shape[0]):
        P = fw.decode_point(C, pts[k])
        assert P is not mm.INF and C.on_curve(P)
        assert fw.in_subgroup(C, P) == bool(ok[k]), k
    if name == "mnt4_g2":
        assert int((ok == 0).sum()) >= 4 and int((ok == 1).sum()) >= 4
    else:
        assert ok.all()   # prime order: is_in_safe_subgroup() is true (mnt4_g1.cpp:425, mnt6_g1.cpp:424)


@pytest.mark.parametrize("name", sorted(fw.MNT_GROUPS))
def test_model_reproduces_recorded_results(name):
    C = fw.MNT_GROUPS[name][0]
    f = fw.fixtures()
    bases = [fw.decode_point(C, b) for b in f[f"{name}/bases"]]
    scalars = [fw.decode_scalar(s) for s in f[f"{name}/scalars"]]
    assert (fw.encode_point(C, C.msm(bases, scalars)) == f[f"{name}/msm_out"]).all()
    A, B, O = (f[f"{name}/add_{x}"] for x in ("a", "b", "out"))
    assert A.shape[0] == 6
    for k in range(A.shape[0]):
        got = C.add(fw.decode_point(C, A[k]), fw.decode_point(C, B[k]))
        assert (fw.encode_point(C, got) == O[k]).all(), k
    zero = fw.encode_point(C, mm.INF)
    assert (O[2] == zero).all() and (O[5] == zero).all() and (O[3] == A[3]).all()   # P + (-P), 0 + 0, P + 0
    Pm, S, O = (f[f"{name}/mul_{x}"] for x in ("p", "s", "out"))
    assert [fw.decode_scalar(s) for s in S[1:]] == [0, 1, C.r - 1]
    for k in range(Pm.shape[0]):
        got = C.mul(fw.decode_scalar(S[k]), fw.decode_point(C, Pm[k]))
        assert (fw.encode_point(C, got) == O[k]).all(), k
    # encode / decode round trip on every recorded element
    for key in ("bases", "add_out", "mul_out", "curve_points"):
        for row in f[f"{name}/{key}"]:
            assert (fw.encode_point(C, fw.decode_point(C, row)) == row).all()
