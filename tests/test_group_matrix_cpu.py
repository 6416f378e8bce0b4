"""Sparse matrix times point vector (amdmsm_group_matrix_apply / _device / amdmsm_plan_group_matrix) as far as a host
without a GPU can see it: the symbols are exported and declared, the Python engine has the methods with their
keyword-only arguments, (MNT6, G2) and an unknown curve are refused before the context is looked at, a group the library
carries asks for a context, and the ABI version is what it was."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_group_matrix_apply", "amdmsm_group_matrix_apply_device", "amdmsm_plan_group_matrix")
BAD_ARG, UNSUPPORTED = -2, -3
CARRIED = [(c, g) for c in (0, 1, 2, 3, 4) for g in (1, 2)] + [(5, 1)]


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def entries(lib, curve, group):
    """the three entries with a null context, a handle that cannot exist and nothing else"""
    z, mat = ctypes.c_size_t(0), ctypes.c_uint64(1)
    return (lib.amdmsm_group_matrix_apply(None, curve, group, mat, None, z, 0, z, None, z, None),
            lib.amdmsm_group_matrix_apply_device(None, curve, group, mat, None, z, None, z, None),
            lib.amdmsm_plan_group_matrix(None, curve, group, mat, z, (ctypes.c_size_t * 8)()))


def test_the_symbols_are_exported_declared_and_listed(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header


def test_engine_has_the_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.group_matrix_apply).parameters
    assert list(host)[:4] == ["self", "mat", "group", "points"]
    assert list(host)[4:] == ["base_form", "out_form", "chunk_entries", "stride_bytes", "out"]
    assert all(host[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(host)[4:])
    assert host["base_form"].default == libff_amd.multi_exp_base_form_normal and host["out_form"].default == libff_amd.OUT_LIBFF
    assert host["chunk_entries"].default == 0 and host["stride_bytes"].default is None and host["out"].default is None
    dev = inspect.signature(libff_amd.Engine.group_matrix_apply_device).parameters
    assert list(dev)[:6] == ["self", "mat", "group", "d_points_affine", "n_points", "d_out_xyz"]
    assert list(dev)[6:] == ["out_form", "chunk_entries", "stream"]
    assert all(dev[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(dev)[6:])
    assert dev["out_form"].default == libff_amd.OUT_LIBFF and dev["chunk_entries"].default == 0 and dev["stream"].default is None
    plan = inspect.signature(libff_amd.Engine.plan_group_matrix).parameters
    assert list(plan) == ["self", "mat", "group", "chunk_entries"] and plan["chunk_entries"].default == 0


def test_mnt6_g2_and_an_unknown_curve_are_refused_before_the_context(lib):
    from libff_amd import G1, G2, MNT6

    assert entries(lib, MNT6, G2) == (UNSUPPORTED,) * 3
    for group in (G1, G2):
        assert entries(lib, 9, group) == (UNSUPPORTED,) * 3
    assert entries(lib, 0, 3) == (UNSUPPORTED,) * 3


@pytest.mark.parametrize("curve,group", CARRIED)
def test_a_carried_group_asks_for_a_context(lib, curve, group):
    assert entries(lib, curve, group) == (BAD_ARG,) * 3
    assert b"ctx" in lib.amdmsm_last_error(None)


def test_the_abi_version_is_unchanged(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    assert "#define AMDMSM_ABI_VERSION 3" in header
    assert lib.amdmsm_abi_version() == 3 == e.ABI_VERSION
