"""The integer model of the coordinate fields (tests/field_model.py) against the reference's recorded field results and
against tests/mnt_model.py, and the coverage of its operand sets: which side of every data-dependent correction of
fp.cuh the operands of tests/test_gpu_field_probe.py take, counted from the model alone (the device is never asked).

Sides recorded as out of reach of operands inside the contract: none.  The second subtraction of 2p after a fused sum
of four products on alt_bn128 (bound 4.03 p) fires for a few dozen of the directed quadruples around 2p - 1 (largest
unreduced value reached: 4.013 p); every other field's sums stay below the bound fp_dot_subs derives.
"""
import random

import numpy as np
import pytest

import field_model as fm
import mnt_model as mm
from common import GROUPS, golden, to_int

MIN_MUL, MIN_OTHER = 64, 16


@pytest.mark.parametrize("name,curve,group", GROUPS)
def test_model_reproduces_the_reference(name, curve, group):
    g, E = golden(), fm.ext(name)
    F = E.F
    assert F.p == to_int(g[f"{name}/fq_modulus"])
    a, b = fm.from_words(F, g[f"{name}/fq_a"], E.deg), fm.from_words(F, g[f"{name}/fq_b"], E.deg)
    for op in ("mul", "sqr", "add", "sub", "neg", "inv"):
        want = fm.from_words(F, g[f"{name}/fq_{op}"], E.deg)
        got = [fm.exact(E, op, (x, y)) for x, y in zip(a, b)]
        assert got == want, op
        assert (fm.to_words(F, got) == g[f"{name}/fq_{op}"]).all(), op


@pytest.mark.parametrize("name", ["mnt4_g1", "mnt4_g2", "mnt6_g1"])
def test_model_agrees_with_the_mnt_model(name):
    E = fm.ext(name)
    F = E.F
    curve = {"mnt4_g1": mm.MNT4, "mnt4_g2": mm.MNT4_G2, "mnt6_g1": mm.MNT6}[name]
    M = curve.F
    assert F.p == curve.p and F.R == mm.RADIX and E.deg == M.deg and (E.deg == 1 or E.nr == M.nr)
    rng = random.Random(5)
    plain = lambda st: M.of_comps([curve.fq_from_mont(c) for c in st])
    stored = lambda v: tuple(curve.fq_mont(c) for c in M.comps(v))
    for _ in range(64):
        a, b = (tuple(rng.randrange(F.p) for _ in range(E.deg)) for _ in range(2))
        assert plain(E.mul(a, b)) == M.mul(plain(a), plain(b))
        assert plain(E.add(a, b)) == M.add(plain(a), plain(b))
        assert plain(E.sub(a, b)) == M.sub(plain(a), plain(b))
        assert plain(E.inv(a)) == M.inv(plain(a))
        assert stored(plain(a)) == a
        assert (fm.to_words(F, [a])[0] == curve._coord_words(plain(a))).all()


@pytest.mark.parametrize("fname", fm.FIELD_NAMES)
def test_montgomery_t_against_a_word_level_cios(fname):
    """the model's closed form of t is what a 32-bit-word CIOS loop produces"""
    F = fm.field(fname)
    rng = random.Random(3)
    for _ in range(50):
        a, b = rng.randrange(2 * F.p), rng.randrange(2 * F.p)
        t = 0
        for i in range(F.N):
            t += ((a >> (32 * i)) & 0xffffffff) * b
            m = (t * F.npinv) & 0xffffffff
            t = (t + m * F.p) >> 32
        assert t == F.mont_t(a, b) and t < 2 * F.p and t % F.p == F.mul(a, b)


def _report(name, op, cnt):
    print(f"{name:13s} {op:15s} " + "; ".join(f"{k}: {v}" for k, v in sorted(cnt.items())))


@pytest.mark.parametrize("name", [g[0] for g in fm.GROUPS])
def test_operands_take_both_sides_of_every_correction(name):
    """Per group: at least 64 operand pairs on each side of the final subtraction of `mul` (prime-field groups, whose
    operands are the field's), at least 16 on each side of every other correction the bound of fp.cuh says can fire."""
    E = fm.ext(name)
    F = E.F
    for op in ("mul", "sqr", "add", "sub", "half", "canon", "add_lz", "sub_lz", "mul_lz", "mul_sub_mul_lz"):
        cnt = fm.sides(name, op)
        _report(name, op, cnt)
        for key, v in cnt.items():
            if key.endswith("max t/p"):
                continue
            need = MIN_MUL if (op == "mul" and key.startswith("mul")) else MIN_OTHER
            assert min(v) >= need, (name, op, key, v)
        if E.deg == 1 and op in ("mul", "sqr"):
            assert "mul t >= p" in cnt
        # every subtraction fp_dot_subs asks for is listed, so that none goes uncounted
        if op == "mul_sub_mul_lz" and E.fused():
            T = 2 if E.deg == 1 else 4
            f2s = {4} if (E.deg == 1 or E.nr == -1) else {4, 20}
            for f2 in f2s:
                for k in range(F.dot_subs(T, f2)):
                    assert f"dot T={T} F2={f2} subtraction {k + 1} of {F.dot_subs(T, f2)}" in cnt


def test_operand_domains_and_determinism():
    for name in ("alt_bn128_g2", "mnt4_g1"):
        E = fm.ext(name)
        for op in fm.OPS:
            bound = (2 if op in fm.LAZY_OPS else 1) * E.F.p
            ops_ = fm.operands(name, op)
            assert all(0 <= c < bound for args in ops_ for e in args for c in e), op
            assert len(ops_[0]) == fm.ARITY.get(op, 1) and all(len(e) == E.deg for e in ops_[0])
            if op in ("inv", "sqrt"):
                assert len(ops_) <= fm.N_SLOW
                sq = [E.is_square(a[0]) for a in ops_]
                assert sum(sq) >= 16 and len(sq) - sum(sq) >= 16
                assert (E.zero(),) not in ops_ or op == "sqrt"
    fm.operands.cache_clear()
    again = fm.operands("mnt4_g1", "mul_sub_mul_lz")
    fm.operands.cache_clear()
    assert again == fm.operands("mnt4_g1", "mul_sub_mul_lz")
