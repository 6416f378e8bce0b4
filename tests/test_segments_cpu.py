"""Segmented MSM (amdmsm_multi_exp_segments / amdmsm_msm_device_segments) as far as a host without a GPU can see it: both
symbols are exported and declared, the Python engine has both methods, (MNT6, G2) is refused before the context is looked
at and a group the library carries asks for one."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_multi_exp_segments", "amdmsm_msm_device_segments")
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
    assert "#define AMDMSM_SEG_SHARED_BASES 1u" in header
    assert e.SEG_SHARED_BASES == 1 and e.SEG_LONG_NEVER == ctypes.c_size_t(-1).value


def test_engine_has_both_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.multi_exp_segments).parameters
    for arg in ("curve", "group", "bases", "scalars", "offsets"):
        assert host[arg].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD, arg
    for arg in ("shared_bases", "long_from", "base_form", "out_form", "scalars_plain", "chunk_terms"):
        assert host[arg].kind == inspect.Parameter.KEYWORD_ONLY, arg
    assert host["shared_bases"].default is False and host["long_from"].default == 0 and host["chunk_terms"].default == 0
    assert host["scalars_plain"].default is False
    dev = inspect.signature(libff_amd.Engine.msm_device_segments).parameters
    for arg in ("curve", "group", "offsets", "shared_bases", "long_from", "out_form", "scalars_plain", "chunk_terms", "stream"):
        assert arg in dev, arg


def test_mnt6_g2_is_refused_and_a_carried_group_asks_for_a_context(lib):
    from libff_amd import G1, G2, MNT6

    z, u = ctypes.c_size_t(0), ctypes.c_uint(0)
    host = lambda group: lib.amdmsm_multi_exp_segments(None, MNT6, group, None, z, 0, z, None, z, None, z, u, z, None, None)
    dev = lambda group: lib.amdmsm_msm_device_segments(None, MNT6, group, None, z, None, z, None, z, u, z, None, None)
    assert host(G2) == UNSUPPORTED and dev(G2) == UNSUPPORTED
    assert host(G1) == BAD_ARG and dev(G1) == BAD_ARG
