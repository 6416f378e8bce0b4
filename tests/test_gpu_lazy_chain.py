"""The Horner chains on loose 28-bit limbs (libff_amd/csrc/wide28.cuh jac_add_28, msm_group.hip horner_chain_lazy) on
the device.

1. tools/lazy_chain_test.hip, built on the box like tools/wide_test.hip: jac_add_28 and mixed chains of jac_dbl_28 /
   jac_add_28 against jac_add_wide / jac_dbl_wide, X, Y and Z word for word after from28, for the three fields of the
   lazy chain -- random points, P + P, P + (-P), P + 0, 0 + P, 0 + 0, coordinates p - 1, p - 2, all-ones words, single
   bits, zero X or Y, chains of up to 22 doublings and 8 additions in random order, 3000 runs per field.
2. End to end, the canonical chain (AMDMSM_HORNER_LAZY=0) and the lazy one in a child process each (the switch is read
   once per process): alt_bn128 G1 and bls12_377 G1, n = 64 and 1000 against port.multi_exp, window_bits 4 (many short
   runs), 10 and 16, endomorphism split off and permitted; the composed inputs of tests/tail_cases.py whose window sums
   (H) and bit planes (HP) are equal, opposite or infinite after their doublings, against the closed form; and
   multi_exp_batch with k = 2 (k_horner_batch).  The child prints one line per case, the parent asserts on the lines;
   after a child that faulted or ran out of time nothing more of this file starts on the device."""
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

import tail_cases as tc  # noqa: E402
from common import GROUPS  # noqa: E402

pytestmark = pytest.mark.gpu

PORT_GROUPS = {g[0]: g for g in GROUPS}
NAMES = ["alt_bn128_g1", "bls12_377_g1"]
SIZES = [64, 1000]
WINDOW_BITS = [4, 10, 16]
_fault = []


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _fault:
        pytest.fail(f"not started: an earlier child of this file faulted or timed out ({_fault[0]})")


def test_loose_limb_chain_selftest(tmp_path):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "lazy_chain_test"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(REPO, "libff_amd", "csrc"),
                    os.path.join(REPO, "tools", "lazy_chain_test.hip"), "-o", str(exe)], check=True, capture_output=True,
                   timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "LAZY CHAIN TEST PASSED" in r.stdout and r.stdout.count("word for word: ok") == 3, r.stdout[-3000:]


def _composed(fam, c):
    return tc.h_cases(fam, c) + tc.hp_cases(fam, c)


def _labels(name):
    """the lines a child has to print, in order"""
    out = [f"random n={n} c={c} endo={e}" for n in SIZES for c in WINDOW_BITS for e in ("off", "on")]
    return out, WINDOW_BITS


def child_main(name):
    import libff_amd
    from libff_amd import multi_exp_base_form_special
    from oracle import port
    port.build()
    fam = tc.PortFamily(port, *PORT_GROUPS[name])
    engine = libff_amd.Engine(0)
    endo_on = 0 if name == "alt_bn128_g1" else 1
    p = port
    for n in SIZES:
        bases = p.bases_seq(fam.curve, fam.group, n, first=11)
        sc = p.scalars_sha512(fam.curve, 1000 + n, n)
        want = fam.msm(bases, sc)
        for c in WINDOW_BITS:
            for label, mode in (("off", -1), ("on", endo_on)):
                engine.endomorphism = mode
                got = engine.multi_exp(fam.curve, fam.group, bases, sc, base_form=multi_exp_base_form_special, window_bits=c)
                print(f"CASE random n={n} c={c} endo={label} {'ok' if (got == want).all() else 'MISMATCH'}", flush=True)
    engine.endomorphism = -1
    for c in WINDOW_BITS:
        for case in _composed(fam, c):
            bases, sc, dlog, _ = tc.materialize(fam, case)
            got = engine.multi_exp(fam.curve, fam.group, bases, sc, base_form=multi_exp_base_form_special, window_bits=c)
            print(f"CASE composed c={c} {case.name} {'ok' if fam.same(got, dlog) else 'MISMATCH'}", flush=True)
        hs = tc.h_cases(fam, c)
        n = max(x.n for x in hs)
        for pair in ((hs[0], hs[1]), (hs[2], hs[5])):
            mats = [tc.materialize(fam, x.padded(n)) for x in pair]
            got = engine.multi_exp_batch(fam.curve, fam.group, [m[0] for m in mats], [m[1] for m in mats],
                                         base_form=multi_exp_base_form_special, window_bits=c)
            ok = all(fam.same(g, m[2]) for g, m in zip(got, mats))
            print(f"CASE batch c={c} {pair[0].name}+{pair[1].name} {'ok' if ok else 'MISMATCH'}", flush=True)
    print("CHILD-DONE", flush=True)


def _wanted(name, port):
    fam = tc.PortFamily(port, *PORT_GROUPS[name])
    want, _ = _labels(name)
    for c in WINDOW_BITS:
        want += [f"composed c={c} {case.name}" for case in _composed(fam, c)]
        hs = tc.h_cases(fam, c)
        want += [f"batch c={c} {a.name}+{b.name}" for a, b in ((hs[0], hs[1]), (hs[2], hs[5]))]
    return want


@pytest.mark.parametrize("lazy", ["0", "1"], ids=["canonical", "lazy"])
@pytest.mark.parametrize("name", NAMES)
def test_horner_chains_end_to_end(port, name, lazy):
    env = dict(os.environ, AMDMSM_HORNER_LAZY=lazy)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _fault.append(f"{name} lazy={lazy}: time limit")
        pytest.fail(f"{name} lazy={lazy}: child ran out of time; last output: {(e.stdout or b'')[-500:]!r}")
    if r.returncode != 0 or "CHILD-DONE" not in r.stdout:
        _fault.append(f"{name} lazy={lazy}: exit status {r.returncode}")
        pytest.fail(f"{name} lazy={lazy}: child ended with status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    lines = set(r.stdout.splitlines())
    want = _wanted(name, port)
    assert len(want) >= 40
    bad = [w for w in want if f"CASE {w} ok" not in lines]
    assert not bad, (name, lazy, bad)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
