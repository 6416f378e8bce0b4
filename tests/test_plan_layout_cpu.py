"""The MSM plan is pinned: what amdmsm_plan_ex and amdmsm_plan_short answer -- (c, W, buckets, workspace_bytes,
endomorphism_used), or the return code of a refusal -- equals tests/golden/plan_layout.json over its whole grid (four
groups, nine lengths, seven window sizes, the split off / on / auto, full-width and short scalars).  The fixture was
taken from a library built before the workspace's regions were given one description each (plan_t's ws_region table in
engine.cpp), so the size of the workspace -- the end of its last region, behind every stride -- has not moved.

The table is taken by tests/golden/make_plan_layout.py in a child process that sees no device, where the resident-lane
query takes its fixed fallback on any machine."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GENERATOR = os.path.join(HERE, "golden", "make_plan_layout.py")
FIXTURE = os.path.join(HERE, "golden", "plan_layout.json")
NAMES = {"0,1": "alt_bn128 G1", "1,2": "bls12_377 G2", "2,1": "bw6_761 G1", "4,1": "mnt4 G1"}


@pytest.fixture(scope="module")
def tables():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    got = json.loads(subprocess.check_output([sys.executable, GENERATOR, libff_amd.engine.SO_PATH], env=env, text=True))
    with open(FIXTURE) as f:
        return got, json.load(f)


def test_grid_is_the_recorded_one(tables):
    got, want = tables
    for key in ("sizes", "window_bits", "endomorphism", "short_bits"):
        assert got[key] == want[key], key
    assert want["sizes"] == [1, 63, 64, 65, 1000, 1 << 16, 3 << 18, 1 << 20, 1 << 23]
    assert want["window_bits"] == [0, 2, 9, 10, 16, 22, 24]
    assert sorted(want["endomorphism"]) == [-1, 0, 1, 2] and want["short_bits"] == [0, 1, 32, 64]
    assert sorted(want["plans"]) == sorted(NAMES) == sorted(got["plans"])


@pytest.mark.parametrize("group", sorted(NAMES))
def test_plans_equal_the_recorded_ones(tables, group):
    got, want = tables
    reqs = [(n, wb, endo, bits) for n in want["sizes"] for wb in want["window_bits"] for endo in want["endomorphism"]
            for bits in want["short_bits"]]
    assert len(got["plans"][group]) == len(want["plans"][group]) == len(reqs)
    plans = refusals = 0
    for req, g, w in zip(reqs, got["plans"][group], want["plans"][group]):
        assert g == w, (f"{NAMES[group]} (n, window_bits, endomorphism, short bits) = {req}: "
                        f"[rc, c, W, buckets, workspace_bytes, endomorphism_used] = {g}, recorded {w}")
        plans += w[0] == 0
        refusals += w[0] != 0
    # the grid holds both kinds: window sizes the short form, the split or the planner refuse, and real plans
    assert plans > 0 and refusals > 0
