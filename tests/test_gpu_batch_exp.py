"""Fixed-base amdmsm_batch_exp at its edges (k_fb_gouter, k_fb_table_level, k_fb_table_affine, k_fb_exp, k_fb_exp_rr and
the resident-table cache of engine.cpp), all eleven groups: table shapes whose last row is full, two entries long or
ragged against the 32 entries one lane normalises; windows 1 to 22; batches at the edges of the 256-lane workgroup;
scalars with zero digits in every position, as Montgomery and as plain records; coefficients 0, 1, r - 1; bases that are
zero, not normalised, of order two or outside the order-r subgroup; and one context driven through a sequence of calls
that reuse, replace and must not confuse its table.

No expectation comes from the device: every element of every result is compared, as an affine point, with the closed
form of tests/fixed_base_cases.py, which tests/test_fixed_base_cases_cpu.py proves against the oracle's batch_exp."""
import random

import numpy as np
import pytest

import fixed_base_cases as fb

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402

BAD_ARG = -2
_groups = {}


def _grp(port, name):
    if name not in _groups:
        _groups[name] = fb.group_of(port, name)
    return _groups[name]


class Expect:
    """closed-form results for one base, one scalar multiplication per distinct multiplier"""

    def __init__(self, grp, g, in_subgroup=True, rule=None):
        self.grp, self.g, self.in_subgroup, self.rule, self.memo = grp, g, in_subgroup, rule, {}

    def keys(self, ks, coeff=None):
        grp = self.grp
        if coeff is not None:
            ks = [coeff * k % grp.r for k in ks]
        if self.rule is not None:
            return grp.keys(self.rule(grp, self.g, ks))
        new = [k for k in dict.fromkeys(ks) if k not in self.memo]
        for k, key in zip(new, grp.keys(fb.closed_form(grp, self.g, new, in_subgroup=self.in_subgroup))):
            self.memo[k] = key
        return [self.memo[k] for k in ks]


def _run(engine, grp, scalar_size, window, g, ks, plain, coeff=None):
    cf = grp.scalars([coeff], plain)[0] if coeff is not None else None
    got = engine.batch_exp(grp.curve, grp.group, scalar_size, window, g, grp.scalars(ks, plain), coeff=cf, scalars_plain=plain)
    assert got.shape[0] == len(ks)
    return grp.keys(got)


def _check(engine, grp, scalar_size, window, g, ks, want, plain, coeff=None):
    """every element, as an affine point"""
    got = _run(engine, grp, scalar_size, window, g, ks, plain, coeff)
    bad = [i for i in range(len(ks)) if got[i] != want[i]]
    assert not bad, (grp.name, scalar_size, window, "plain" if plain else "montgomery", coeff, len(bad), bad[:8],
                     [hex(ks[i]) for i in bad[:4]])


def _both_forms(engine, grp, scalar_size, window, g, exp, n, seed):
    """the edge scalars of the shape as Montgomery records (values below r) and as plain records (any value below
    2^scalar_size: without a coefficient the kernel takes the digits of the integer as it stands)"""
    for plain in (False, True):
        ks = fb.scalar_values(scalar_size, window, grp.r, seed, n, below_r=not plain or not exp.in_subgroup or exp.rule is not None)
        _check(engine, grp, scalar_size, window, g, ks, exp.keys(ks), plain)


SHAPE_IDS = ["b-w1", "b-w2", "64-w16", "65-w16", "1-w1", "maxsize-w13", "b-w17"]
SHAPE_N = [513, 513, 256, 255, 257, 257, 256]


@pytest.mark.parametrize("shape", range(len(SHAPE_IDS)), ids=SHAPE_IDS)
@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_table_shapes(engine, port, name, shape):
    """2 b entries ragged against 32; window 2; a last row that is full and one of two entries; one row of two entries;
    the largest scalar_size; the shape bench.py times.  g is the generator."""
    grp = _grp(port, name)
    scalar_size, window = fb.table_shapes(grp.bits, grp.limbs)[shape]
    exp = Expect(grp, grp.one)
    _both_forms(engine, grp, scalar_size, window, grp.one, exp, SHAPE_N[shape], seed=shape)
    if scalar_size == 1:   # n = 1 as well: one lane, one digit
        for k in (0, 1):
            for plain in (False, True):
                _check(engine, grp, 1, 1, grp.one, [k], exp.keys([k]), plain)


@pytest.mark.parametrize("scalar_size", [23, 22], ids=["two-rows", "one-full-row"])
@pytest.mark.parametrize("name", ["alt_bn128_g1", "mnt4_g1"])
def test_largest_window(port, name, scalar_size):
    """window 22 through k_fb_exp_rr and k_fb_exp; the table is grow-only context memory, hence a context of its own"""
    grp = _grp(port, name)
    eng = libff_amd.Engine(0)
    try:
        _both_forms(eng, grp, scalar_size, 22, grp.one, Expect(grp, grp.one), 257, seed=scalar_size)
    finally:
        eng.close()


@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_coefficients(engine, port, name):
    """batch_exp_with_coeff: 0 (every result zero), 1, r - 1 (the negatives), a random one; Montgomery and plain records,
    where the plain path converts both factors before it multiplies"""
    grp = _grp(port, name)
    g = grp.multiple_not_normalised(1234567)
    exp = Expect(grp, g)
    rnd = random.Random(11).randrange(2, grp.r - 1)
    for scalar_size, window in ((grp.bits, 4), (64 * grp.limbs, 13)):
        ks = fb.scalar_values(scalar_size, window, grp.r, seed=window, n=255, below_r=True)
        plain_results = fb.closed_form(grp, g, ks)
        want = {0: grp.keys([grp.zero] * len(ks)), 1: exp.keys(ks), grp.r - 1: grp.keys([grp.neg(x) for x in plain_results])}
        assert want[1] == grp.keys(plain_results)
        if window == 4:
            want[rnd] = exp.keys(ks, coeff=rnd)
        for coeff, keys in want.items():
            for plain in (False, True):
                _check(engine, grp, scalar_size, window, g, ks, keys, plain, coeff=coeff)


@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_bases_zero_and_not_normalised(engine, port, name):
    grp = _grp(port, name)
    g = grp.multiple_not_normalised(987654321)
    for scalar_size, window in ((grp.bits, 5), (65, 16)):
        _both_forms(engine, grp, scalar_size, window, g, Expect(grp, g), 257, seed=window)
        zero = Expect(grp, grp.zero, rule=lambda gr, t, ks: [gr.zero] * len(ks))
        _both_forms(engine, grp, scalar_size, window, grp.zero, zero, 257, seed=window)


@pytest.mark.parametrize("name", ["bls12_377_g1", "bw6_761_g1"])
def test_base_of_order_two(engine, port, name):
    """g = (-1, 0) / (1, 0): g for an odd multiplier, zero for an even one; the table build doubles into infinity and
    every row after the first is infinite"""
    grp = _grp(port, name)
    t = grp.order_two()
    exp = Expect(grp, t, rule=fb.order_two_rule)
    for window in (1, 3, 5):
        _both_forms(engine, grp, grp.bits, window, t, exp, 257, seed=window)
    ks = fb.scalar_values(grp.bits, 5, grp.r, seed=5, n=257, below_r=True)
    for plain in (False, True):
        _check(engine, grp, grp.bits, 5, t, ks, exp.keys(ks, coeff=12345), plain, coeff=12345)


@pytest.mark.parametrize("name", [n for n in fb.ALL_GROUPS if n not in ("alt_bn128_g1", "mnt4_g1", "mnt6_g1")])
def test_base_outside_the_subgroup(engine, port, name):
    """a curve point whose order is not r: out[i] is the integer multiple v_i g"""
    grp = _grp(port, name)
    p = grp.outside_subgroup()
    assert p is not None
    exp = Expect(grp, p, in_subgroup=False)
    for window in (1, 3, 5):
        _both_forms(engine, grp, grp.bits, window, p, exp, 257, seed=7)


def test_groups_without_a_point_outside_the_subgroup(port):
    for name in ("alt_bn128_g1", "mnt4_g1", "mnt6_g1"):
        assert _grp(port, name).outside_subgroup() is None


@pytest.mark.parametrize("name,other", [("alt_bn128_g1", "mnt4_g1"), ("bls12_377_g2", "bw6_761_g1")])
def test_one_context_one_sequence(port, name, other):
    """The resident table over a sequence of calls on one context: reused for the same (group, scalar_size, window, g),
    rebuilt for anything else -- another window, -g (same X), another group -- untouched by a refused call and by the
    entries that share the scalar and output buffers.  Reuse shows in ms[1], the time between two adjacent events when
    nothing is built: below a tenth of what the build of the same table took."""
    grp, grp2 = _grp(port, name), _grp(port, other)
    b = grp.bits
    g1, g2 = grp.multiple_not_normalised(31337), grp.multiple_not_normalised(4242)
    e1, e1n, e2 = Expect(grp, g1), Expect(grp, grp.neg(g1)), Expect(grp, g2)
    eng = libff_amd.Engine(0)
    try:
        def step(label, gr, scalar_size, window, g, exp, n, seed, plain=False):
            ks = fb.scalar_values(scalar_size, window, gr.r, seed, n, below_r=True) if n else []
            got = _run(eng, gr, scalar_size, window, g, ks, plain)
            ms = eng.batch_exp_timings()   # amdmsm_get_batch_exp_timings: ms[1] is "table_ms"
            print(f"{name} {label}: n={len(ks)} ms={ {k: round(v, 4) for k, v in ms.items()} }")
            want = exp.keys(ks)
            bad = [i for i in range(len(ks)) if got[i] != want[i]]
            assert not bad, (label, len(bad), bad[:8])
            return ms["table_ms"]

        build13 = step("1 build (g1, b, 13)", grp, b, 13, g1, e1, 257, seed=1)
        reuse13 = step("2 same table, other scalars", grp, b, 13, g1, e1, 257, seed=2, plain=True)
        assert reuse13 < build13 / 10, (reuse13, build13)
        step("3 (g1, b, 12)", grp, b, 12, g1, e1, 257, seed=3)
        step("4 (-g1, b, 12): same X, negated Y", grp, b, 12, grp.neg(g1), e1n, 257, seed=3)
        build9 = step("5a n = 0 builds (g2, b, 9)", grp, b, 9, g2, e2, 0, seed=0)
        reuse = step("5b reuses it", grp, b, 9, g2, e2, 257, seed=5)
        assert reuse < build9 / 10, (reuse, build9)
        # 6: refused calls leave the output, the error text and the table alone
        ks = [1, 2, 3, grp.r - 1]
        for scalar_size, window in ((b, 0), (b, 23), (0, 9), (64 * grp.limbs + 1, 9)):
            out = np.full((4, grp.one.shape[0]), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                eng.batch_exp(grp.curve, grp.group, scalar_size, window, g2, grp.scalars(ks, False), out=out)
            assert ei.value.code == BAD_ARG and "window / scalar_size" in str(ei.value), (scalar_size, window, str(ei.value))
            assert eng.lib.amdmsm_last_error(eng.h).decode() == "window / scalar_size"
            assert (out == 0xA5A5A5A5A5A5A5A5).all(), (scalar_size, window)
        reuse = step("7 reuses it after the refusals", grp, b, 9, g2, e2, 257, seed=7, plain=True)
        assert reuse < build9 / 10, (reuse, build9)
        # 8: the entries that share the scalar buffer and the output buffer of batch_exp
        if isinstance(grp, fb.OracleGroup):
            c, gid, n = grp.curve, grp.group, 300
            bases, sc = port.bases_seq(c, gid, n, first=40), port.scalars_sha512(c, 800, n)
            want = port.multi_exp(c, gid, bases, sc, port.BDLO12_SIGNED, 1)
            assert (eng.multi_exp(c, gid, bases, sc, base_form=libff_amd.multi_exp_base_form_special) == want).all()
            got = eng.scalar_mul_vec(c, gid, bases, sc, base_form=libff_amd.multi_exp_base_form_special)
            muls = [port.scalar_mul(c, gid, bases[i], sc[i]) for i in range(n)]
            assert grp.keys(got) == grp.keys(muls)
            half = n // 2
            got = eng.fold_vec(c, gid, [bases[:half], bases[half:]], sc[:2], base_form=libff_amd.multi_exp_base_form_special)
            fold = [port.group_op(c, gid, 0, port.scalar_mul(c, gid, bases[i], sc[0]), port.scalar_mul(c, gid, bases[half + i], sc[1]))
                    for i in range(half)]
            assert grp.keys(got) == grp.keys(fold)
        reuse = step("9 reuses it after the other entries", grp, b, 9, g2, e2, 513, seed=9)
        assert reuse < build9 / 10, (reuse, build9)
        step("10 another group", grp2, grp2.bits, 9, grp2.one, Expect(grp2, grp2.one), 257, seed=10)
        step("11 the first group again", grp, b, 9, g2, e2, 257, seed=11)
    finally:
        eng.close()
