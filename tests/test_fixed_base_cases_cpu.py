"""The expectations of tests/test_gpu_batch_exp.py (tests/fixed_base_cases.py) proven without a device: the closed form
out[i] = (coeff) v_i g against the oracle's batch_exp -- libff's get_window_table and windowed_exp restated
(oracle/msm_oracle.c, pinned to the reference by test_oracle_vs_ref.py) -- and, for the MNT groups, against the same
double loop written over the integer model."""
import random

import pytest

import fixed_base_cases as fb
import mnt_model as mm
from common import GROUP_IDS

MNT_IDS = ["mnt4_g1", "mnt4_g2", "mnt6_g1"]


def _oracle_keys(grp, scalar_size, window, g, ks, coeff=None):
    cf = grp.scalars([coeff], False)[0] if coeff is not None else None
    return grp.keys(grp.port.batch_exp(grp.curve, grp.group, scalar_size, window, g, grp.scalars(ks, False), coeff=cf))


@pytest.mark.parametrize("name", GROUP_IDS)
def test_closed_form_is_the_oracles_batch_exp(port, name):
    grp = fb.group_of(port, name)
    g = grp.multiple_not_normalised(77)
    for scalar_size, window in ((grp.bits, 3), (65, 16), (1, 1)):
        ks = fb.scalar_values(scalar_size, window, grp.r, seed=scalar_size, below_r=True)
        want = _oracle_keys(grp, scalar_size, window, g, ks)
        assert grp.keys(fb.closed_form(grp, g, ks)) == want, (scalar_size, window)
        # a coefficient keeps the product below 2^scalar_size only when it is 1, or when the table covers all of Fr
        if window < 16:   # (the oracle builds its table entry by entry: once is enough for the large one)
            assert grp.keys(fb.closed_form(grp, g, ks, coeff=1)) == _oracle_keys(grp, scalar_size, window, g, ks, coeff=1)
    ks = fb.scalar_values(grp.bits, 3, grp.r, seed=9, below_r=True)[::4]
    for coeff in (0, grp.r - 1, random.Random(3).randrange(grp.r)):
        got = grp.keys(fb.closed_form(grp, g, ks, coeff=coeff))
        assert got == _oracle_keys(grp, grp.bits, 3, g, ks, coeff=coeff), coeff
        if coeff == 0:
            assert got == grp.keys([grp.zero] * len(ks))
    neg = grp.keys([grp.neg(x) for x in fb.closed_form(grp, g, ks)])
    assert grp.keys(fb.closed_form(grp, g, ks, coeff=grp.r - 1)) == neg


@pytest.mark.parametrize("name", ["bls12_377_g1", "bw6_761_g1"])
def test_order_two_rule(port, name):
    """g of order two: g for an odd multiplier and zero for an even one, every table row after the first infinite"""
    grp = fb.group_of(port, name)
    t = grp.order_two()
    for window in (1, 3, 5):
        ks = fb.scalar_values(grp.bits, window, grp.r, seed=window, below_r=True)
        assert grp.keys(fb.order_two_rule(grp, t, ks)) == _oracle_keys(grp, grp.bits, window, t, ks), window
    coeff = 12345
    assert grp.keys(fb.order_two_rule(grp, t, ks, coeff)) == _oracle_keys(grp, grp.bits, 5, t, ks, coeff=coeff)


@pytest.mark.parametrize("name", GROUP_IDS)
def test_outside_subgroup_expectation(port, name):
    """a curve point outside the order-r subgroup: the integer multiple, nothing reduced mod r"""
    grp = fb.group_of(port, name)
    p = grp.outside_subgroup()
    if p is None:   # the whole curve group has order r (alt_bn128 G1): there is no such point
        assert name == "alt_bn128_g1"
        return
    assert grp.keys([grp.mul(grp.r - 1, p, in_subgroup=False)]) != grp.keys([grp.neg(p)]), "r p is zero: p is in the subgroup"
    for window in (1, 3, 5):
        ks = fb.scalar_values(grp.bits, window, grp.r, seed=window, below_r=True)
        assert grp.keys(fb.closed_form(grp, p, ks, in_subgroup=False)) == _oracle_keys(grp, grp.bits, window, p, ks), window


def _windowed_exp_model(model, scalar_size, window, g, k):
    """get_window_table and windowed_exp (multiexp.tcc:809-872) as they stand, over affine model points"""
    outerc = (scalar_size + window - 1) // window
    table, gouter = [], g
    for length in fb.row_lengths(scalar_size, window):
        row, ginner = [], mm.INF
        for _ in range(length):
            row.append(ginner)
            ginner = model.add(ginner, gouter)
        table.append(row)
        for _ in range(window):
            gouter = model.add(gouter, gouter)
    res = table[0][0]
    for outer in range(outerc):
        inner = 0
        for i in range(window):
            if (k >> (outer * window + i)) & 1:
                inner |= 1 << i
        res = model.add(res, table[outer][inner])
    return res


@pytest.mark.parametrize("name", MNT_IDS)
def test_mnt_closed_form_is_the_windowed_loop(port, name):
    grp = fb.group_of(port, name)
    model = grp.model
    bases = [(grp.multiple_not_normalised(5), True)]
    if grp.outside_subgroup() is not None:
        bases.append((grp.outside_subgroup(), False))
    for g, sub in bases:
        P = model.point(g)
        for scalar_size, window in ((grp.bits, 3), (65, 4), (1, 1), (grp.bits, 1)):
            ks = fb.scalar_values(scalar_size, window, grp.r, seed=window, below_r=True)
            ks = ks[:-8:9] + ks[-8:]   # every ninth edge value, and the random ones
            want = [_windowed_exp_model(model, scalar_size, window, P, k) for k in ks]
            assert grp.keys(fb.closed_form(grp, g, ks, in_subgroup=sub)) == want, (scalar_size, window)
    ks = [0, 1, grp.r - 1, 987654321]
    got = grp.keys(fb.closed_form(grp, grp.one, ks, coeff=grp.r - 1))
    assert got == [model.neg(model.mul(k, model.one)) for k in ks]
    assert grp.keys([grp.zero]) == [mm.INF]


@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_scalar_values_hold_the_edges(port, name):
    grp = fb.group_of(port, name)
    for scalar_size, window in fb.table_shapes(grp.bits, grp.limbs) + [(23, 22), (22, 22)]:
        rows = fb.row_lengths(scalar_size, window)
        assert sum(rows) <= ((scalar_size + window - 1) // window) << window and rows[-1] >= 2
        for below_r in (False, True):
            n = 513 if window <= 2 else 257
            ks = fb.scalar_values(scalar_size, window, grp.r, seed=1, n=n, below_r=below_r)
            assert len(ks) == n and all(0 <= k < 1 << scalar_size for k in ks)
            assert not below_r or all(k < grp.r for k in ks)
            for k in ks:   # no digit indexes past its row: the contract of batch_exp
                assert all(d < length for d, length in zip(fb.digits(k, scalar_size, window), rows))
            assert 0 in ks and 1 in ks
            for j in range(len(rows)):   # one nonzero digit: the lowest and the highest bit of every window
                for k in (j * window, j * window + window - 1):
                    assert (1 << k in ks) == (k < scalar_size and not (below_r and 1 << k >= grp.r)), k
            top = (1 << scalar_size) - 1
            assert (top in ks) == (not below_r or top < grp.r)
            if scalar_size >= grp.bits:
                assert grp.r - 1 in ks
            if len(rows) > 2:
                assert any(k and fb.digits(k, scalar_size, window)[:2] == [0, 0] for k in ks)
                for phase in (0, 1):   # zero and nonzero digits in turn, up to the highest nonzero one
                    alt = [k for k in ks if k >> window and all(
                        (d != 0) == (j % 2 == phase)
                        for j, d in enumerate(fb.digits(k, k.bit_length(), window)))]
                    assert alt, ("no value with alternating zero / nonzero digits", phase)
