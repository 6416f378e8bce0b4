"""Equal, opposite and empty operands through every adder behind k_accumulate, on the device.  The inputs come from
tests/tail_cases.py (what each aims at and why it fires whatever the summation order is: there); tests/test_tail_cases_cpu.py
proves on the host that they are what they claim.  Every result must equal the closed form (sum_i k_i m_i) G bit for bit in
affine form -- for the MNT groups as the point of tests/mnt_model.py -- and, for the groups of the C oracle, port.multi_exp.

Matrix: all eight groups of common.GROUPS and the three MNT groups; c in {4, 7, 9} (segment path) and {10, 11, 12, 13}
(row / column sums, even and odd column bits; all of them take k_plane_sums_wide, whose narrow sibling k_plane_sums is
reached by the AMDMSM_PLANES_WIDE=0 and AMDMSM_ROWCOL_MIN_C children); c = 13 is left to the 8- to 12-word prime-field G1
groups -- the Fq2 groups and the 24-word field stop at 12.  Every input runs with the endomorphism split off (the digits
are then the planned ones) and once more with it permitted (no coverage claim, the value must hold); the MNT groups ignore
the option (test_gpu_mnt.py) and run once.  The precomputed-table entry reads libff's on-disk records, which only the C
oracle writes: the eight oracle groups.

The reduction knobs are read once per process, so each alternative tail path runs in a child process of this very file
(`python test_gpu_tail_cases.py --child ...`) under its own time limit; the child prints one line per case and the parent
asserts on the lines.  One engine and one child at a time.  After a child that faulted, aborted or ran out of time every
later test of this file fails at once instead of starting more work on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mnt_model as mm  # noqa: E402
import tail_cases as tc  # noqa: E402
from common import GROUPS  # noqa: E402

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, OUT_JACOBIAN, multi_exp_base_form_special  # noqa: E402

MNT_GROUPS = {"mnt4_g1": (libff_amd.MNT4, 1, mm.MNT4), "mnt4_g2": (libff_amd.MNT4, 2, mm.MNT4_G2),
              "mnt6_g1": (libff_amd.MNT6, 1, mm.MNT6)}
PORT_GROUPS = {g[0]: g for g in GROUPS}
ALL_GROUPS = list(PORT_GROUPS) + list(MNT_GROUPS)
NARROW = ("alt_bn128_g1", "bls12_377_g1", "bls12_381_g1", "mnt4_g1", "mnt6_g1")   # 8- to 12-word prime-field G1


def cs_for(name):
    return tc.SEGMENT_CS + [c for c in tc.ROWCOL_CS if c <= 12 or name in NARROW]


_fams = {}
_fault = []


def family(name, port=None):
    if name not in _fams:
        if name in MNT_GROUPS:
            _fams[name] = tc.MntFamily(name, *MNT_GROUPS[name])
        else:
            if port is None:
                from oracle import port
                port.build()
            _fams[name] = tc.PortFamily(port, *PORT_GROUPS[name])
    return _fams[name]


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _fault:
        pytest.fail(f"not started: an earlier child of this file faulted or timed out ({_fault[0]})")


def _endo_modes(name):
    if name in MNT_GROUPS:
        return [-1]
    return [-1, 0 if name == "alt_bn128_g1" else 1]


def run_case(engine, fam, case, modes=(-1,), oracle=True, **kw):
    """list of failure descriptions of one input"""
    bases, sc, dlog, desc = tc.materialize(fam, case)
    fails = []
    saved = engine.endomorphism
    try:
        for mode in modes:
            engine.endomorphism = mode
            got = engine.multi_exp(fam.curve, fam.group, bases, sc, base_form=multi_exp_base_form_special,
                                   window_bits=kw.get("window_bits", case.c), **{k: v for k, v in kw.items() if k != "window_bits"})
            if not fam.same(got, dlog):
                fails.append(f"{fam.name} c={case.c} {case.name} endomorphism={mode}: not the closed form")
            if oracle and isinstance(fam, tc.PortFamily) and case.n <= 1 << 16 and mode == -1:
                p = fam.port
                want = p.multi_exp(fam.curve, fam.group, bases, sc, p.BDLO12_SIGNED, p.FORM_SPECIAL, chunks=8, omp=True) \
                    if case.n >= 4096 else fam.msm(bases, sc)
                if not (got == want).all():
                    fails.append(f"{fam.name} c={case.c} {case.name}: differs from port.multi_exp")
    finally:
        engine.endomorphism = saved
    return fails


MATRIX = [pytest.param(name, c, f, id=f"{name}-c{c}-{f}") for name in ALL_GROUPS for c in cs_for(name) for f in tc.FAMILIES]


@pytest.mark.parametrize("name,c,fam_name", MATRIX)
def test_tail_cases(engine, port, name, c, fam_name):
    fam = family(name, port)
    assert libff_amd.plan(fam.curve, fam.group, 1000, window_bits=c, endomorphism=-1)["num_windows"] == tc.num_windows(fam, c)
    fails = []
    for case in tc.cases_for(fam, c, fam_name):
        fails += run_case(engine, fam, case, _endo_modes(name))
    assert not fails, fails


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_377_g1"])
def test_wide_windows_and_planner_choice(engine, port, name):
    """c = 16 (U, U with the top bucket, A_0, A_14, F forms), and U at 2^18 points with the planner's own window size"""
    fam = family(name, port)
    fails = []
    c = 16
    for case in (tc.u_case(fam, c), tc.u_case(fam, c, top=True), tc.a_case(fam, c, 0), tc.a_case(fam, c, c - 2)):
        fails += run_case(engine, fam, case, _endo_modes(name))
    n = 1 << 18
    c = libff_amd.plan(fam.curve, fam.group, n, endomorphism=-1)["c"]
    copies = n // (1 << (c - 1))
    case = tc.u_case(fam, c, copies=copies)
    assert n - (1 << (c - 1)) * 2 < case.n <= n
    case = case.padded(n)
    fails += run_case(engine, fam, case, _endo_modes(name), oracle=False, window_bits=0)
    assert not fails, fails


@pytest.mark.parametrize("c", [7, 11])
@pytest.mark.parametrize("name", ALL_GROUPS)
def test_batches_of_uniform_and_sign_patterns(engine, port, name, c):
    """U, A_0 (k = 2) and U, A_0, A_(c-2) (k = 3) through multi_exp_batch: the tail kernels run once over all windows"""
    fam = family(name, port)
    cases = [tc.u_case(fam, c), tc.a_case(fam, c, 0), tc.a_case(fam, c, c - 2)]
    mats = [tc.materialize(fam, x) for x in cases]
    saved = engine.endomorphism
    engine.endomorphism = -1
    try:
        for k in (2, 3):
            got = engine.multi_exp_batch(fam.curve, fam.group, [m[0] for m in mats[:k]], [m[1] for m in mats[:k]],
                                         base_form=multi_exp_base_form_special, window_bits=c)
            assert [fam.same(g, m[2]) for g, m in zip(got, mats)] == [True] * k, (k, [x.name for x in cases[:k]])
    finally:
        engine.endomorphism = saved


@pytest.mark.parametrize("c", [10, 12])
@pytest.mark.parametrize("name", ALL_GROUPS)
def test_batched_horner_chains(engine, port, name, c):
    """the k chains of k_horner_batch with a different H pattern each (k = 2 and 3)"""
    fam = family(name, port)
    hs = tc.h_cases(fam, c)
    n = max(x.n for x in hs)
    saved = engine.endomorphism
    engine.endomorphism = -1
    try:
        for group_of in ([hs[0], hs[1]], [hs[2], hs[1], hs[4]], [hs[5], hs[3], hs[0]], [hs[2], hs[2]]):
            mats = [tc.materialize(fam, x.padded(n)) for x in group_of]
            got = engine.multi_exp_batch(fam.curve, fam.group, [m[0] for m in mats], [m[1] for m in mats],
                                         base_form=multi_exp_base_form_special, window_bits=c)
            assert [fam.same(g, m[2]) for g, m in zip(got, mats)] == [True] * len(mats), [x.name for x in group_of]
    finally:
        engine.endomorphism = saved


@pytest.mark.parametrize("c", [7, 10])
@pytest.mark.parametrize("name", list(PORT_GROUPS))
def test_uniform_buckets_through_precomputed_table(engine, port, name, c, tmp_path):
    """U through the one-window path of multi_exp_stream_with_precompute: every digit of every window lands in ONE bucket set,
    where the bucket of weight d holds the Wu points 2^(cw) P -- all bucket sums are equal again"""
    fam = family(name, port)
    case = tc.u_case(fam, c)
    bases, sc, dlog, desc = tc.materialize(fam, case)
    assert libff_amd.precompute_num_digits(fam.curve, c) >= case.meta["windows"]
    tab = engine.precompute_table(fam.curve, fam.group, bases, c)
    path = tmp_path / "table.bin"
    path.write_bytes(port.disk_write(fam.curve, fam.group, tab).tobytes())
    got = engine.multi_exp_stream_with_precompute_file(fam.curve, fam.group, str(path), sc, c)
    assert fam.same(got, dlog), desc


@pytest.mark.parametrize("name", ALL_GROUPS)
def test_horner_patterns_through_split_chunks(engine, port, name):
    """H with chunks = 3, split_chunks = True: three partial MSMs whose results -- equal, opposite or infinite by
    construction of the patterns -- go through k_sum_points"""
    fam = family(name, port)
    fails = []
    for case in tc.h_cases(fam, 10):
        fails += run_case(engine, fam, case, oracle=False, chunks=3, split_chunks=True)
    assert not fails, fails


@pytest.mark.parametrize("name", ALL_GROUPS)
def test_sum_points_equal_opposite_infinite(engine, port, name):
    """engine.sum_points on lists whose neighbours (and halves) are equal, opposite or at infinity"""
    fam = family(name, port)
    saved = engine.endomorphism
    engine.endomorphism = -1
    try:
        jac = {}
        for m in sorted({v for lst in tc.SUM_POINT_LISTS for v in lst}, key=str):
            base = fam.point(1 if m is None else m)[None, :]
            jac[m] = engine.multi_exp(fam.curve, fam.group, base, fam.scalars_mont([0 if m is None else 1]),
                                      base_form=multi_exp_base_form_special, out_form=OUT_JACOBIAN)
        for lst in tc.SUM_POINT_LISTS:
            got = engine.sum_points(fam.curve, fam.group, np.stack([jac[m] for m in lst]), out_form=OUT_AFFINE)
            assert fam.same(got, sum(v or 0 for v in lst)), lst
    finally:
        engine.endomorphism = saved


# ------------------------------------------------------------------ alternative tail paths, one child process each
KNOBS = {
    "rowcol_off": ({"AMDMSM_ROWCOL": "0"}, [12]),                                          # segment kernels at c = 12
    "planes_narrow": ({"AMDMSM_PLANES_WIDE": "0"}, [10, 11]),                              # k_plane_sums
    "q1": ({"AMDMSM_ROWCOL_QROW": "1", "AMDMSM_ROWCOL_QCOL": "1"}, [10, 11]),              # pure butterfly
    "q64": ({"AMDMSM_ROWCOL_QROW": "64", "AMDMSM_ROWCOL_QCOL": "64"}, [10, 11]),           # pure serial (clamped to the length)
    "acc_s16": ({"AMDMSM_ACC_S": "16"}, [9, 11]),                                          # pins the span classes of F
    "rowcol_min_c": ({"AMDMSM_ROWCOL_MIN_C": "7"}, [7, 9]),                                # planes below / at the wide threshold
}
KNOB_GROUPS = ["alt_bn128_g1", "bls12_377_g2", "bw6_761_g1"]


def _child_lines(name, cs):
    fam = family(name)
    return [(c, case) for c in cs for case in tc.knob_cases(fam, c)]


def child_main(name, cs):
    from oracle import port
    port.build()
    fam = family(name, port)
    engine = libff_amd.Engine(0)
    engine.endomorphism = -1
    for c, case in _child_lines(name, cs):
        fails = run_case(engine, fam, case, oracle=False)
        print(f"CASE {name} c={c} {case.name} {'ok' if not fails else 'MISMATCH'}", flush=True)
    print("CHILD-DONE", flush=True)


@pytest.mark.parametrize("name", KNOB_GROUPS)
@pytest.mark.parametrize("knob", list(KNOBS))
def test_alternative_tail_paths(port, knob, name):
    env_extra, cs = KNOBS[knob]
    family(name, port)
    env = dict(os.environ, **env_extra)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + [str(c) for c in cs]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        _fault.append(f"{knob} {name}: time limit")
        pytest.fail(f"{knob} {name}: child ran out of time; last output: {(e.stdout or b'')[-500:]!r}")
    if r.returncode != 0 or "CHILD-DONE" not in r.stdout:
        _fault.append(f"{knob} {name}: exit status {r.returncode}")
        pytest.fail(f"{knob} {name}: child ended with status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    lines = set(r.stdout.splitlines())
    want = [f"CASE {name} c={c} {case.name}" for c, case in _child_lines(name, cs)]
    assert len(want) >= 20
    bad = [w for w in want if w + " ok" not in lines]
    assert not bad, (knob, bad)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2], [int(x) for x in sys.argv[3:]])
