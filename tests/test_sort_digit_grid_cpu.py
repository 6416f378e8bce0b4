"""The block and grid rule of the sort's digit pass (group_vtable.h sort_digit_grid, read through
amdmsm_plan_sort_digit_grid -- the function msm_group.hip sort_launch itself asks), without a device: walking the blocks the
way the kernels do -- workgroup g takes blocks g, g + grid, ..., thread t of a block takes item block_index * block + t --
must visit every work item exactly once, start no block at or past the end and launch no idle workgroup."""
import ctypes

import numpy as np
import pytest

import libff_amd
from libff_amd.engine import load_library

NS = [0, 1, 1023, 1024, 1025, 5000, 1 << 20, (1 << 20) + 1]
GRIDS = [1, 2, 3, 512]


def tpb():
    """the digit pass's workgroup size (group_vtable.h SORT_DIGIT_TPB): the block of an input that fills any grid"""
    return libff_amd.plan_sort_digit_grid(1 << 40, 1)["block"]


def walk(items, g):
    """visits per item, and the block starts, of the kernels' loop"""
    block, blocks, grid = g["block"], g["blocks"], g["grid"]
    visits = np.zeros(items, dtype=np.int64)
    starts = []
    for wg in range(grid):
        mine = np.arange(wg, blocks, grid, dtype=np.int64)   # this workgroup's blocks
        assert len(mine) >= 1, "a workgroup without a block was launched"
        starts += list(mine * block)
        idx = (mine[:, None] * block + np.arange(block, dtype=np.int64)[None, :]).ravel()   # block * block_size + thread
        np.add.at(visits, idx[idx < items], 1)
    return visits, starts


@pytest.mark.parametrize("wgs", GRIDS)
@pytest.mark.parametrize("n", NS)
def test_scalar_blocks_cover_every_index_once(n, wgs):
    g = libff_amd.plan_sort_digit_grid(n, wgs)
    assert g["block"] == tpb()   # scalars: whole workgroups, so the digit columns are written a workgroup's width in a row
    assert g["blocks"] == (n + tpb() - 1) // tpb()
    assert g["grid"] == min(g["blocks"], wgs)
    visits, starts = walk(n, g)
    assert (visits == 1).all()
    assert all(s < n for s in starts) and len(set(starts)) == g["blocks"]


def packed_items(n, wb, misalign):
    """work items of n packed integers of wb bytes whose vector starts `misalign` bytes past a 16-byte boundary
    (msm_group.hip packed_split): whole 16-byte vectors plus the single elements in front of and behind them"""
    epl = 16 // wb
    head = min(((16 - misalign) // wb) if misalign else 0, n)
    nvec = (n - head) // epl
    return nvec + (n - nvec * epl)


@pytest.mark.parametrize("wgs", GRIDS)
@pytest.mark.parametrize("wb", [1, 2, 4, 8])
@pytest.mark.parametrize("n", NS)
def test_packed_item_blocks_cover_every_item_once(n, wb, wgs):
    for misalign in (0, wb):
        items = packed_items(n, wb, misalign % 16)
        assert items <= n and (n == 0) == (items == 0)
        g = libff_amd.plan_sort_digit_grid(items, wgs, block_min=256)
        assert 256 <= g["block"] <= tpb() and g["block"] & (g["block"] - 1) == 0
        assert g["blocks"] == (items + g["block"] - 1) // g["block"] and g["grid"] == min(g["blocks"], wgs)
        # a block shrinks only while whole workgroups' worth of items would leave a part of the device without one
        if g["block"] < tpb():
            assert (items + 2 * g["block"] - 1) // (2 * g["block"]) < wgs
        if g["block"] > 256:
            assert g["blocks"] >= wgs
        visits, starts = walk(items, g)
        assert (visits == 1).all()
        assert all(s < items for s in starts) and len(set(starts)) == g["blocks"]


def test_flagship_and_large_grids():
    """2^20 scalars on 512 resident workgroups: two blocks each, 512 merges instead of 1024; 2^26: 128 blocks each"""
    g = libff_amd.plan_sort_digit_grid(1 << 20, 512)
    assert (g["block"], g["blocks"], g["grid"]) == (tpb(), (1 << 20) // tpb(), 512)
    g = libff_amd.plan_sort_digit_grid(1 << 26, 512)
    assert (g["block"], g["blocks"], g["grid"]) == (tpb(), (1 << 26) // tpb(), 512)
    # item counts past 2^32 keep their block count (the kernels index blocks with 64 bits)
    g = libff_amd.plan_sort_digit_grid((1 << 33) + 5, 512)
    assert g["blocks"] == (1 << 33) // tpb() + 1 and g["grid"] == 512


def test_arguments():
    out = (ctypes.c_size_t * 3)()
    lib = load_library()
    assert lib.amdmsm_plan_sort_digit_grid(ctypes.c_size_t(10), 0, 0, out) == -2   # no workgroups: AMDMSM_ERR_BAD_ARG
    assert lib.amdmsm_plan_sort_digit_grid(ctypes.c_size_t(10), 0, 4, None) == -2
    # a block_min above the workgroup size means the workgroup size
    assert libff_amd.plan_sort_digit_grid(5000, 3, block_min=4096) == libff_amd.plan_sort_digit_grid(5000, 3)
