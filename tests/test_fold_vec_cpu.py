"""Fold of point vectors (amdmsm_fold_vec / _device / amdmsm_plan_fold) as far as a host without a GPU can see it: the
symbols are exported and declared, the Python engine has the methods, (MNT6, G2) is refused, and the plan follows the
permission rule of the endomorphism split."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_fold_vec", "amdmsm_fold_vec_device", "amdmsm_plan_fold")
BAD_ARG, UNSUPPORTED = -2, -3
PAIRING = [(c, g) for c in (0, 1, 2, 3) for g in (1, 2)]   # alt_bn128, bls12_377, bw6_761, bls12_381: G1, G2
MNT = [(4, 1), (4, 2), (5, 1)]


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


def test_engine_has_the_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.fold_vec).parameters
    assert list(host)[:5] == ["self", "curve", "group", "points_list", "scalars"]
    for arg in ("base_form", "out_form", "scalars_plain", "chunk_points"):
        assert arg in host, arg
    assert host["out_form"].default == libff_amd.OUT_LIBFF and host["scalars_plain"].default is False
    assert host["chunk_points"].default == 0 and host["base_form"].default == libff_amd.multi_exp_base_form_normal
    dev = inspect.signature(libff_amd.Engine.fold_vec_device).parameters
    assert list(dev)[:7] == ["self", "curve", "group", "d_points_list", "scalars", "n", "d_out_xyz"]
    for arg in ("out_form", "scalars_plain", "chunk_points", "stream"):
        assert arg in dev, arg
    assert dev["out_form"].default == libff_amd.OUT_LIBFF and dev["scalars_plain"].default is False
    assert dev["chunk_points"].default == 0 and dev["stream"].default is None
    assert "plan_fold" in libff_amd.__all__ and callable(libff_amd.plan_fold)


def test_mnt6_g2_is_refused(lib):
    """the group the library does not carry is refused before the context is looked at; a group it carries asks for one"""
    from libff_amd import G1, G2, MNT6

    z = ctypes.c_size_t(0)
    host = lambda group: lib.amdmsm_fold_vec(None, MNT6, group, 2, None, z, 0, None, z, None, z, None)
    dev = lambda group: lib.amdmsm_fold_vec_device(None, MNT6, group, 2, None, None, z, None, z, None)
    assert host(G2) == UNSUPPORTED and dev(G2) == UNSUPPORTED
    assert host(G1) == BAD_ARG and dev(G1) == BAD_ARG
    out = (ctypes.c_size_t * 5)()
    assert lib.amdmsm_plan_fold(MNT6, G2, 2, z, z, 0, out) == UNSUPPORTED


def test_plan_rows_follow_the_permission_rule(lib):
    from libff_amd import plan_fold

    for curve, group in PAIRING + MNT:
        for k in (1, 2, 8):
            p = plan_fold(curve, group, k, 1000, endomorphism=-1)
            assert p["rows"] == k and not p["endomorphism"], (curve, group, k)
    # 0: only where the whole curve group has order r
    p = plan_fold(0, 1, 3, 1000, endomorphism=0)
    assert p["rows"] == 6 and p["endomorphism"]
    assert not plan_fold(0, 2, 3, 1000, endomorphism=0)["endomorphism"]
    assert not plan_fold(1, 1, 3, 1000, endomorphism=0)["endomorphism"]
    # 1 / 2: the caller's guarantee -- at every size, there is no cost model
    for value in (1, 2):
        for n in (1, 1000, 1 << 24):
            p = plan_fold(1, 1, 3, n, endomorphism=value)
            assert p["rows"] == 6 and p["endomorphism"], (value, n)
    for curve, group in MNT:
        for value in (-1, 0, 1, 2):
            p = plan_fold(curve, group, 2, 1000, endomorphism=value)
            assert p["rows"] == 2 and not p["endomorphism"], (curve, group, value)


def test_plan_windows(lib):
    """without the split: the ladder's digits of the group (one more than the scalar's words hold, for the carry), which
    the segmented MSM uses too; with it: fewer, and enough for the bound of the half scalars"""
    from libff_amd import endomorphism_info, plan_fold, sizes

    for curve, group in PAIRING + MNT:
        full = plan_fold(curve, group, 2, 1000, endomorphism=-1)["num_windows"]
        bits = sizes(curve, group)["fr_bytes"] * 8
        w = 4                                          # msm_group.hip SMV_W
        assert full == bits // w + 1, (curve, group)   # SMV_DIGITS: whole windows over the words, plus the carry digit
        if (curve, group) in PAIRING:
            split = plan_fold(curve, group, 2, 1000, endomorphism=2)["num_windows"]
            assert split < full
            assert w * split - 1 > endomorphism_info(curve, group)["bound_log2"]   # the top digit cannot carry out
            assert split <= (full + 1) // 2 + 1


def test_plan_chunks(lib):
    from libff_amd import plan_fold, sizes

    for curve, group in PAIRING + MNT:
        aff = sizes(curve, group)["affine_bytes"]
        for k in (1, 2, 8):
            p = plan_fold(curve, group, k, 1 << 30)
            assert p["chunk_points"] % 256 == 0 and p["chunk_points"] >= 256, (curve, group, k)
            assert p["workspace_bytes"] <= 1 << 30
            assert p["workspace_bytes"] >= 8 * (k + 1) * aff * p["chunk_points"]   # k tables and one table of scratch
            # the next multiple of 256 would not fit
            assert p["workspace_bytes"] + 256 * 8 * (k + 1) * aff > 1 << 30
            assert plan_fold(curve, group, k, 100)["chunk_points"] == 100          # never more than there is
            assert plan_fold(curve, group, k, 1000, chunk_points=64)["chunk_points"] == 64
            assert plan_fold(curve, group, k, 10, chunk_points=64)["chunk_points"] == 10


def test_plan_refuses_k_out_of_range(lib):
    out = (ctypes.c_size_t * 5)()
    z = ctypes.c_size_t(1000)
    for k in (0, 9, -1):
        assert lib.amdmsm_plan_fold(0, 1, k, z, ctypes.c_size_t(0), 0, out) == BAD_ARG
    assert lib.amdmsm_plan_fold(0, 1, 8, z, ctypes.c_size_t(0), 0, out) == 0
