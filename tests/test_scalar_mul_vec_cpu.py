"""Element-wise scalar multiplication (amdmsm_scalar_mul_vec / _device) as far as a host without a GPU can see it: both
symbols are exported and declared, the Python engine has both methods, and (MNT6, G2) is refused."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_scalar_mul_vec", "amdmsm_scalar_mul_vec_device")
BAD_ARG, UNSUPPORTED = -2, -3


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def test_both_symbols_are_exported_and_declared(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header


def test_engine_has_both_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.scalar_mul_vec).parameters
    for arg in ("curve", "group", "points", "scalars", "base_form", "out_form", "scalars_plain", "chunk_points"):
        assert arg in host, arg
    assert host["scalars_plain"].default is False and host["chunk_points"].default == 0
    dev = inspect.signature(libff_amd.Engine.scalar_mul_vec_device).parameters
    for arg in ("curve", "group", "out_form", "scalars_plain", "chunk_points", "stream"):
        assert arg in dev, arg


def test_mnt6_g2_is_refused(lib):
    """the group the library does not carry is refused before the context is looked at; a group it carries asks for one"""
    from libff_amd import G1, G2, MNT6

    z = ctypes.c_size_t(0)
    host = lambda group: lib.amdmsm_scalar_mul_vec(None, MNT6, group, None, z, 0, None, z, None, z, None)
    dev = lambda group: lib.amdmsm_scalar_mul_vec_device(None, MNT6, group, None, None, z, None, z, None)
    assert host(G2) == UNSUPPORTED and dev(G2) == UNSUPPORTED
    assert host(G1) == BAD_ARG and dev(G1) == BAD_ARG
