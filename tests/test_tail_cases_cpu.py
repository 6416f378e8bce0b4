"""The constructions of tests/tail_cases.py are what they claim -- no device needed.  For every builder, group family and
window size the device file uses: (a) libff's signed recoding of every composed scalar gives the planned digit in every
window, the carry of the 2^(c-1) digit included; (b) the stated property holds on the discrete logs (all bucket values
equal; every pair of buckets opposite in some A_j; the running Horner value equal to +- the next addend; the plane
collisions; the sparse layouts); (c) the C oracle's multi_exp -- mnt_model.msm on the small inputs of the MNT groups --
equals the closed form.  This file is the witness that tests/test_gpu_tail_cases.py tests what it says."""
import itertools

import numpy as np
import pytest

import mnt_model as mm
import tail_cases as tc
from common import GROUPS

# Fr depends on the curve only: digits and properties are checked once per curve, values once per group
CURVE_REP = {0: GROUPS[0], 1: GROUPS[2], 2: GROUPS[4], 3: GROUPS[6]}
MNT = [("mnt4_g1", 4, 1, mm.MNT4), ("mnt4_g2", 4, 2, mm.MNT4_G2), ("mnt6_g1", 5, 1, mm.MNT6)]
ALL_CS = tc.SEGMENT_CS + tc.ROWCOL_CS
_fams = {}


def port_family(port, name, curve, group):
    if name not in _fams:
        _fams[name] = tc.PortFamily(port, name, curve, group)
    return _fams[name]


def mnt_family(name, curve, group, model):
    if name not in _fams:
        _fams[name] = tc.MntFamily(name, curve, group, model)
    return _fams[name]


def all_cases(fam, c):
    return [case for f in tc.FAMILIES for case in tc.cases_for(fam, c, f)]


def check_digits(fam, case, port=None, seen=None):
    """(a): the planned digits are the recoding of the composed scalars (Python restatement; and the oracle's own
    orc_signed_digit where the curve has one)"""
    rows = {}
    for row, k in zip(case.digits.tolist(), case.scalars()):
        rows[k] = row
    for k, row in rows.items():
        assert 0 <= k < fam.r, case.name
        assert tc.signed_digits(k, case.c, case.W) == row, (case.name, k)
        if port is not None and (case.c, k) not in seen:
            seen.add((case.c, k))
            plain = tc._limbs([k], fam.fl)[0]
            assert [port.signed_digit(fam.curve, plain, case.c, w) for w in range(case.W)] == row, (case.name, k)


def check_property(fam, case):
    """(b)"""
    r, c, m = fam.r, case.c, case.meta
    B = 1 << (c - 1)
    bv = case.bucket_values(r)
    kind = m["kind"]
    if kind == "U":
        want = {(w, d) for w in range(m["windows"]) for d in range(1, B + (1 if m["top"] else 0))}
        body = {k: v for k, v in bv.items() if k[0] < m["windows"]}
        assert set(body) == want
        assert set(body.values()) == {m["value"] % r}                 # every bucket sum the same point
        sums = case.window_sums(r)
        assert len(set(sums[:m["windows"]])) == 1                     # the final Horner meets 2^c S + S
    elif kind == "A":
        sums = case.window_sums(r)
        assert all(s == m["window_sum"] % r for s in sums[:m["windows"]])   # the closed form of a window
        assert all(s == 0 for s in sums[m["windows"]:])
        assert all(v in (tc.P0 % r, -tc.P0 % r) for v in bv.values())
    elif kind == "F":
        for w in range(m["windows"]):
            assert sum(1 for k in bv if k[0] == w) == 1               # one bucket per window
        assert (case.digits == case.digits[0]).all()
    elif kind == "H":
        sums = case.window_sums(r)
        top = m["steps"][0][0]
        assert all(s == 0 for s in sums[top + 1:])
        run = 0
        for w, op, before, add in m["steps"]:
            run = run * (1 << c) % r
            assert run == before and sums[w] == add % r
            if op == "=":
                assert run != 0 and sums[w] == run                    # the addition is a doubling
            elif op == "-":
                assert run != 0 and (sums[w] + run) % r == 0          # ... gives infinity
            elif op == ".":
                assert sums[w] == 0
            else:
                assert sums[w] != 0 and sums[w] != run and (sums[w] + run) % r != 0
            run = (run + sums[w]) % r
        assert run == m["result"] == case.expected(r)
        if "-" in [s[1] for s in m["steps"]]:
            zero_then_empty = any(a[1] == "-" and b[1] == "." for a, b in zip(m["steps"], m["steps"][1:]))
            assert zero_then_empty or m["steps"][-1][1] == "-"
    elif kind == "HP":
        for w, k, dist, low in m["plan"]:
            here = {wt: v for (ww, wt), v in bv.items() if ww == w}
            assert set(here) == {1 << k, 1 << (k + dist)}
            assert here[1 << (k + dist)] == 1
            assert here[1 << k] == low % r and abs(low) == 1 << dist  # 2^dist Q meets +-2^dist Q after dist doublings
        ks = sorted(k for _, k, _, _ in m["plan"])
        assert len(set(ks)) == len(ks)
    elif kind == "HPsparse":
        per_w = {}
        for (w, wt) in bv:
            per_w.setdefault(w, []).append(wt)
        assert per_w[0] == [B] and all(len(v) == 1 for v in per_w.values())
        assert any(w not in per_w for w in range(max(per_w)))         # an empty window in between
    elif kind == "Z":
        for w, k, weights in m["layout"]:
            here = sorted(wt for (ww, wt) in bv if ww == w)
            if k == "top":
                assert here == [B] and sorted(wt for (ww, wt) in bv if ww == w + 1) == [1]
            else:
                assert here == sorted(weights)
    else:
        raise AssertionError(kind)


def check_a_family_pairs(fam, c):
    """every pair of weights is an opposite pair in at least one A_j (and an equal pair in the others): exhaustively up to
    c = 8, on all pairs that differ in one bit above"""
    r, B = fam.r, 1 << (c - 1)
    vals = []
    for j in range(c - 1):
        bv = tc.a_case(fam, c, j).bucket_values(r)
        vals.append([None] + [bv[(0, d)] for d in range(1, B)])
    if c <= 8:
        pairs = itertools.combinations(range(1, B), 2)
    else:
        pairs = ((d, d ^ (1 << b)) for d in range(1, B) for b in range(c - 1) if d < d ^ (1 << b) < B)
    for d, e in pairs:
        opp = [j for j in range(c - 1) if (vals[j][d] + vals[j][e]) % r == 0]
        eq = [j for j in range(c - 1) if vals[j][d] == vals[j][e]]
        assert opp and len(opp) + len(eq) == c - 1, (c, d, e)


# (c = 16 runs on alt_bn128 G1 and bls12_377 G1 only)
@pytest.mark.parametrize("curve,c", [(curve, c) for curve in (0, 1, 2, 3) for c in ALL_CS] + [(0, 16), (1, 16)])
def test_digits_and_properties(port, curve, c):
    fam = port_family(port, *CURVE_REP[curve])
    assert tc.num_windows(fam, c) > tc.full_windows(fam, c) >= 3
    seen = set()
    cases = all_cases(fam, c) if c != 16 else [tc.u_case(fam, c), tc.u_case(fam, c, top=True), tc.a_case(fam, c, 0), tc.a_case(fam, c, 14)]
    for case in cases:
        check_digits(fam, case, port, seen)
        check_property(fam, case)
    if c != 16:
        check_a_family_pairs(fam, c)
    assert any(m for m in (case.meta.get("plan") for case in cases) if m) or c == 16
    if c != 16:   # every plane distance and every k occurs
        for dist in (1, 4):
            ks = sorted(k for case in cases for _, k, d, low in case.meta.get("plan", []) if d == dist and low > 0)
            assert ks == list(range(max(0, c - dist))), (dist, ks)


# (the Fq2 groups and the 24-word field stop at c = 12: header of tail_cases.py)
@pytest.mark.parametrize("name,curve,group,model,c", [(*g, c) for g in MNT for c in ALL_CS if c <= 12 or g[2] == 1],
                         ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_digits_and_properties_mnt(name, curve, group, model, c):
    fam = mnt_family(name, curve, group, model)
    if group == 1:   # Fr of a curve once; MNT4 G2 shares MNT4's
        for case in all_cases(fam, c):
            check_digits(fam, case)
            check_property(fam, case)
        check_a_family_pairs(fam, c)
    # (c) on the small inputs: the model's affine sums
    for case in tc.h_cases(fam, c) + tc.hp_cases(fam, c):
        pts = [fam._affine(m) for m in case.dlogs()]
        assert model.msm(pts, case.scalars()) == fam._affine(case.expected(fam.r)), case.name


@pytest.mark.parametrize("name,curve,group,c", [(*g, c) for g in GROUPS for c in ALL_CS if c <= 12 or (g[2] == 1 and g[1] != 2)])
def test_oracle_multi_exp_equals_closed_form(port, name, curve, group, c):
    """(c): port.multi_exp == (sum_i k_i m_i) G for every input (all have n <= 2^16)"""
    fam = port_family(port, name, curve, group)
    for case in all_cases(fam, c):
        assert case.n <= 1 << 16
        bases, sc, dlog, desc = tc.materialize(fam, case)
        got = port.multi_exp(curve, group, bases, sc, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True) \
            if case.n >= 4096 else fam.msm(bases, sc)
        assert fam.same(got, dlog), desc


def test_sum_point_lists():
    for lst in tc.SUM_POINT_LISTS:
        assert lst and all(v is None or isinstance(v, int) for v in lst)
    flat = [tuple(x) for x in tc.SUM_POINT_LISTS]
    assert (5, 5) in flat and (5, -5) in flat and (None, None) in flat
