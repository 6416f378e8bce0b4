"""libff_amd/build.py's per-group compiler flags are pinned: the macro -> value map of every group equals a literal
recorded from the successive edits the table replaced, AMDMSM_EXTRA_FLAGS still replaces a group's own setting of the
same macro, and the compile jobs honour MAX_JOBS and stay within what a job on a shared machine may use."""
import pytest

from libff_amd import build

COMMON = {"AMDMSM_HOT_INLINE": "1", "AMDMSM_BENCH_BOTH": "1"}
RECORDED = {
    "alt_bn128_g1": {"AMDMSM_OVERLAP_OK": "1", "AMDMSM_COLD_INLINE": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "3"},
    "alt_bn128_g2": {"AMDMSM_ACC_SPLIT": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "3"},
    "bls12_377_g1": {"AMDMSM_COLD_INLINE": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "bls12_377_g2": {"AMDMSM_ACC_SPLIT": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "bw6_761_g1": {"AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "bw6_761_g2": {"AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "bls12_381_g1": {"AMDMSM_COLD_INLINE": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "bls12_381_g2": {"AMDMSM_ACC_SPLIT": "1", "AMDMSM_ACC_RR": "1", "AMDMSM_ACC_WAVES": "2"},
    "mnt4_g1": {"AMDMSM_COLD_INLINE": "1", "AMDMSM_ACC_WAVES": "3"},
    "mnt4_g2": {"AMDMSM_ACC_WAVES": "2"},
    "mnt6_g1": {"AMDMSM_COLD_INLINE": "1", "AMDMSM_ACC_WAVES": "3"},
}


def macros(flags):
    """{macro: value} of a list of -DNAME=VALUE flags; a macro given twice or anything else is an error"""
    out = {}
    for f in flags:
        assert f.startswith("-D") and "=" in f, f
        name, value = f[2:].split("=", 1)
        assert name not in out, f"{name} is set twice"
        out[name] = value
    return out


def test_every_group_has_a_row():
    assert list(build.GROUP_FLAGS) == build.GROUPS and sorted(RECORDED) == sorted(build.GROUPS) and len(build.GROUPS) == 11


@pytest.mark.parametrize("group", sorted(RECORDED))
def test_group_flags_are_the_recorded_ones(group):
    assert macros(build.GROUP_FLAGS[group]) == {**COMMON, **RECORDED[group]}
    assert macros(build.group_flags(group)) == {**COMMON, **RECORDED[group]}


@pytest.mark.parametrize("group", ["alt_bn128_g1", "mnt4_g2"])
def test_extra_flag_replaces_the_groups_own_setting(group):
    extra = ["-DAMDMSM_ACC_WAVES=4", "-DAMDMSM_TAIL_WAVES=2"]
    flags = build.group_flags(group, extra)
    assert flags[-2:] == extra   # appended, behind the group's own
    assert macros(flags) == {**COMMON, **RECORDED[group], "AMDMSM_ACC_WAVES": "4", "AMDMSM_TAIL_WAVES": "2"}
    assert macros(build.GROUP_FLAGS[group])["AMDMSM_ACC_WAVES"] == RECORDED[group]["AMDMSM_ACC_WAVES"]   # the table is not edited


def test_build_jobs(monkeypatch):
    monkeypatch.setattr(build.os, "cpu_count", lambda: 384)
    monkeypatch.delenv("MAX_JOBS", raising=False)
    assert build.build_jobs(19) == 16 and build.build_jobs(3) == 3
    monkeypatch.setenv("MAX_JOBS", "4")
    assert build.build_jobs(19) == 4 and build.build_jobs(2) == 2
    monkeypatch.setenv("MAX_JOBS", "64")
    assert build.build_jobs(19) == 16
    for bad in ("", "0", "many"):
        monkeypatch.setenv("MAX_JOBS", bad)
        assert build.build_jobs(19) == 16
    monkeypatch.delenv("MAX_JOBS")
    monkeypatch.setattr(build.os, "cpu_count", lambda: 8)
    assert build.build_jobs(19) == 7
    monkeypatch.setattr(build.os, "cpu_count", lambda: None)
    assert build.build_jobs(19) == 1
