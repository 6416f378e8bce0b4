"""The integer model of the reduced-radix layer (tests/rr_model.py) against plain modular arithmetic, and the coverage of
the operand sets tests/test_gpu_rr_probe.py feeds the device, counted from the model alone (the device is never asked):
every set holds both sides of every branch it is meant to reach, no operand leaves what the callee allows as input, and the
extreme sets are extreme -- their worst column reaches half of what the Checker of tests/test_rr_bounds.py allows for that
product shape.  CPU only."""
from collections import Counter

import pytest

import rr_model as rm
import test_rr_bounds as tb

FQ_UNITS = ["alt_bn128_g1", "bls12_377_g1", "bls12_381_g1", "bw6_761_g1"]
FQ2_UNITS = ["alt_bn128_g2", "bls12_377_g2", "bls12_381_g2"]
PRODUCTS = ("mul", "mul2", "sqr", "re_mul", "re_sqr", "re_mul_sub_mul")


def product_form(s, limbs):
    return all(0 <= l <= s.M for l in limbs[:-1]) and rm.fits_i32(limbs)


def sums_of(u, op, args):
    """the integers S of the product scans one element runs, per component, from plain arithmetic on the operands' values"""
    s, nr = u.s, u.nr
    V = [[rm.value(s, c) for c in e] for e in args]
    if op in ("mul", "sqr", "mul2"):
        if op == "mul":
            return [V[0][c] * V[1][c] for c in range(u.deg)]
        if op == "sqr":
            return [V[0][c] ** 2 for c in range(u.deg)]
        return [V[0][c] * V[1][c] + V[2][c] * V[3][c] for c in range(u.deg)]
    x = V[0]
    y = V[0] if op == "re_sqr" else V[1]
    if u.deg == 1:
        S = [x[0] * y[0]]
        if op == "re_mul_sub_mul":
            S[0] -= V[2][0] * V[3][0]
        return S
    S = [x[0] * y[0] + nr * x[1] * y[1], x[0] * y[1] + x[1] * y[0]]
    if op == "re_mul_sub_mul":
        c, d = V[2], V[3]
        S = [S[0] - c[0] * d[0] - nr * c[1] * d[1], S[1] - c[0] * d[1] - c[1] * d[0]]
    return S


@pytest.mark.parametrize("name", FQ_UNITS + FQ2_UNITS)
def test_products_against_modular_arithmetic(name):
    """residue, range and form of every product the model predicts, on the operand sets of the probe"""
    u = rm.unit(name)
    s, p = u.s, u.s.p
    for op in PRODUCTS:
        two_sums = op == "re_mul_sub_mul" and u.deg == 2 and not s.fits(2.0 * (1.0 + abs(u.nr)))
        for args in rm.limb_operands(name, op)["args"]:
            out, _, _ = rm.limb_expected(name, op, args)
            for c, S in enumerate(sums_of(u, op, args)):
                v = rm.value(s, out[c])
                assert (v * s.rho - S) % p == 0, (name, op, "residue")
                assert rm.fits_i32(out[c])
                if two_sums:   # u - v carried once: two products' ranges, limbs within one carry of B bits
                    assert all(-1 <= l <= s.M + 1 for l in out[c][:-1]), (name, op, "form")
                    continue
                assert 0 <= v * s.rho - S < p * s.rho, (name, op, "range: (S / rho, S / rho + p)")
                assert product_form(s, out[c]), (name, op, "form")


@pytest.mark.parametrize("name", FQ_UNITS + FQ2_UNITS)
def test_linear_ops_and_conversions(name):
    u = rm.unit(name)
    s, p = u.s, u.s.p
    rinv = pow(1 << (32 * s.N), -1, p)
    for op in rm.unit_ops(name):
        if op in PRODUCTS or op == "cneg":
            continue
        for args in rm.limb_operands(name, op)["args"]:
            out, outw, flag = rm.limb_expected(name, op, args)
            for c in range(u.deg):
                a = args[0][c]
                v = rm.value(s, out[c])
                assert rm.fits_i32(out[c]), (name, op)
                if op in ("norm", "ripple"):
                    assert v == rm.value(s, a)
                    # one carry of an int32 limb is within 2^(31 - B): [-4, 2^B + 4) for 29-bit limbs, [-8, 2^B + 8) for 28
                    cmax = 1 << (31 - s.B)
                    lim = (-cmax, s.M + cmax) if op == "norm" else (0, s.M)
                    assert all(lim[0] <= l <= lim[1] for l in out[c][:-1]), (name, op)
                    if op == "norm":
                        assert 0 <= out[c][0] <= s.M
                elif op.startswith("small_times"):
                    cmax = 1 << (31 - s.B)
                    assert v == int(op[-1]) * rm.value(s, a) and all(-cmax <= l <= s.M + cmax for l in out[c][:-1])
                elif op in ("mul_pow2_32n", "mul_pow2_32n_d"):
                    e = 32 * s.N - (s.D if op.endswith("_d") else 0)
                    assert (v * s.rho - (rm.value(s, a) << e)) % p == 0 and product_form(s, out[c])
                    assert 0 <= v * s.rho - (rm.value(s, a) << e) < p * s.rho
                elif op == "from_words_0":
                    assert v == a and product_form(s, out[c]) and out[c][-1] >= 0
                elif op == "from_words_d":
                    assert v == a << s.D and product_form(s, out[c]) and 0 <= out[c][-1] <= s.M
                elif op == "from_words_rho":
                    assert v % p == a * rinv * s.rho % p and 0 <= v < 2 * p and product_form(s, out[c])
                elif op == "first_reduced":
                    assert v % p == (a << s.D) % p and 0 <= v < 2 * p and all(abs(l) <= s.M for l in out[c]), (name, op)
                elif op == "first_coord":
                    assert v % p == (a << s.D) % p and 0 <= v < (2 * p if s.first_needs_reduction(u.nr if u.deg == 2 else 0) else p << s.D)
                elif op == "to_words":
                    assert outw[c] == rm.value(s, a) < p
                elif op == "canon_product":
                    assert 0 <= v < p and v % p == rm.value(s, a) % p and product_form(s, out[c])
                elif op in ("export_0", "export_d"):
                    sh = s.D if op == "export_d" else 0
                    assert 0 <= outw[c] < p and (outw[c] * s.rho - (rm.value(s, a) << (32 * s.N - sh))) % p == 0
                elif op in ("set_pow2_bl", "set_pow2_bl_d"):
                    e = s.BL + (s.D if op.endswith("_d") else 0)
                    assert v == (pow(2, e, p) if c == 0 else 0)
            if op == "is_zero_exact":
                assert bool(flag) == all(rm.value(s, a) % p == 0 for a in args[0]), (name, "every zero in the set lies within J")
            elif op.startswith("maybe_zero"):
                K = s.K if op == "maybe_zero_k" else 64
                for a in args[0]:
                    if rm.value(s, a) % p == 0 and abs(rm.value(s, a) // p) < K:
                        assert rm.maybe_zero(s, a, K), (name, op, "false negative")


@pytest.mark.parametrize("name", FQ_UNITS + FQ2_UNITS + ["bw6_761_g2"])
def test_operands_stay_inside_what_the_code_allows(name):
    u = rm.unit(name)
    s = u.s
    for op in rm.unit_ops(name):
        o = rm.limb_operands(name, op)
        if op in rm.WORD_OPS:
            assert all(0 <= w < s.p for a in o["args"] for w in a[0]), (name, op, "words below p")
            continue
        lim = rm.factor_limit(name, op)
        for args in o["args"]:
            for e in args:
                assert len(e) == u.deg and all(len(c) == s.L for c in e)
                assert all(-lim <= l <= lim for c in e for l in c), (name, op, "limb outside the callee's input range")
        if op in ("norm", "ripple") or op.startswith("small_times"):   # the carry into a limb must not leave int32
            k = o["k"] or 1
            assert all(abs(k * l) < 2 ** 31 for args in o["args"] for c in args[0] for l in c), (name, op)
            assert all(rm.fits_i32(c) for args in o["args"] for c in rm.limb_expected(name, op, args)[0]), (name, op)
        if op in ("export_0", "export_d"):   # rm.export_value asserts the intermediate lies in (-p, 2p)
            [rm.limb_expected(name, op, a) for a in o["args"]]
    for cases, keys in ((rm.madd_cases(name), ("acc",)), (rm.add_cases(name), ("a", "b")), (rm.dbl_cases(name), ("a",)),
                        (rm.jac_cases(name), ("a", "q"))):
        for c in cases:
            for k in keys:
                if c.get(k) is None:
                    continue
                assert all(rm.fits_i32(comp) for e in c[k] for comp in e)
                # every coordinate a point function multiplies is a factor
                assert all(abs(l) <= s.fmax for e in c[k] for comp in e for l in comp[:-1]), (name, k, "factor limbs")


@pytest.mark.parametrize("fname", rm.FIELDS)
def test_branch_sides_of_the_limb_sets(fname):
    s = rm.shape(fname)
    # rr_canon_product and the export behind it: negative, >= p, neither
    name = fname + "_g1"
    sides = Counter(rm.canon_side(s, a[0][0]) for a in rm.limb_operands(name, "canon_product")["args"])
    assert min(sides[k] for k in ("negative", "ge_p", "neither")) >= 32, sides
    for op in ("export_0", "export_d"):
        e = 32 * s.N - (s.D if op == "export_d" else 0)
        sides = Counter(rm.canon_side(s, rm.mul_pow2(s, a[0][0], e)) for a in rm.limb_operands(name, op)["args"])
        assert min(sides[k] for k in ("negative", "ge_p", "neither")) >= 16, (op, sides)
    # rr_first_reduced: the top-word estimate exact and one short (found by search in the model)
    fs = rm.first_sides(s, rm.first_words(fname))
    assert fs["exact"] >= 32 and fs["one_short"] >= 32, fs
    # the zero tests: J per field, j of both signs, every K +- 1, each spread differently; the filter's three outcomes
    J = rm.zero_j_limit(s)
    reps = rm.zero_reps(fname)
    assert J >= s.K + 1, "every |j| the filters are asked about has a representative on int32 limbs"
    assert rm.fits_i32(rm.limbs_of(s, J * s.p)) and not (rm.fits_i32(rm.limbs_of(s, (J + 1) * s.p)) and J + 1 < 1 << (s.B - 1))
    js = {j for _, j, kind in reps if kind == "zero"}
    for K in (64, s.K):
        assert {K - 1, K, K + 1, -(K - 1), -K, -(K + 1)} <= js, (K, sorted(js))
    assert {0, 1, -1, 2, -2, J, -J} <= js
    per_j = Counter(j for _, j, kind in reps if kind == "zero")
    assert min(per_j.values()) >= 4, "each j in several spreads"
    assert any(min(f[:-1]) < 0 for f, _, kind in reps if kind == "zero"), "negative low limbs"
    for K in (64, s.K):
        cnt = rm.filter_sides(s, K, reps)
        assert cnt["false_negative"] == 0 and min(cnt["pass_zero"], cnt["pass_nonzero"], cnt["no_pass"]) >= 8, (K, cnt)
    # ... and the exact test: zero, near miss, same low limb
    ex = Counter((kind, rm.is_zero_exact(s, f)) for f, _, kind in reps)
    assert ex[("zero", True)] >= 64 and ex[("miss", False)] >= 64 and ex[("low_limb", False)] >= 16, ex
    assert ex[("zero", False)] == 0 and ex[("miss", True)] == 0 and ex[("low_limb", True)] == 0, ex


@pytest.mark.parametrize("name", FQ2_UNITS)
def test_branch_sides_of_the_pair_flags(name):
    """the pair-uniform flags: true in both components, in one only, in neither"""
    s = rm.unit(name).s
    for op, fn in (("is_zero_exact", lambda a: rm.is_zero_exact(s, a)), ("maybe_zero_k", lambda a: rm.maybe_zero(s, a, s.K)),
                   ("maybe_zero_64", lambda a: rm.maybe_zero(s, a, 64))):
        cnt = Counter((fn(a[0][0]), fn(a[0][1])) for a in rm.limb_operands(name, op)["args"])
        assert min(cnt[k] for k in ((True, True), (True, False), (False, True), (False, False))) >= 8, (name, op, cnt)


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_rungs_of_the_ladders(name):
    u = rm.unit(name)
    s = u.s
    madd = Counter((c["rung"], c["state"]) for c in rm.madd_cases(name))
    for state in ("first", "steady"):
        for rung in ("general", "same", "opposite", "order_two"):
            assert madd[(rung, state)] >= 4, (name, rung, state, madd)
    assert madd[("first", "first")] >= 8 and madd[("point_inf", "steady")] >= 8 and madd[("point_inf", "first")] >= 1
    assert {c["neg"] for c in rm.madd_cases(name) if c["rung"] in ("same", "opposite")} == {False, True}
    # same x directly after a first point: P = j p with |j| up to 2^D - 1 (1 where the first point is reduced), both
    # signs of j over the set
    js = {"first": [], "steady": []}
    for c in rm.madd_cases(name):
        if c["rung"] in ("same", "opposite", "order_two"):
            j = rm.madd_same_x_multiple(name, c)
            assert j is not None and all(abs(x) < s.K for x in j), (name, "outside the filter's promise")
            js[c["state"]] += j
    reduced = s.first_needs_reduction(u.nr if u.deg == 2 else 0)
    assert max(abs(j) for j in js["first"]) == (1 if reduced else (1 << s.D) - 1), (name, js["first"])
    assert min(js["first"] + js["steady"]) < 0 < max(js["first"] + js["steady"])
    add = Counter(c["rung"] for c in rm.add_cases(name))
    assert min(add[k] for k in ("general", "equal", "opposite", "a_inf", "b_inf", "equal_order_two")) >= 2, add
    eq = Counter((c["rung"], c["sa"], c["sb"]) for c in rm.add_cases(name))
    for rung in ("general", "equal", "opposite"):
        for sa in ("record", "sum"):
            for sb in ("record", "sum"):
                assert eq[(rung, sa, sb)] >= 2, (name, rung, sa, sb)
    dbl = Counter(c["rung"] for c in rm.dbl_cases(name))
    assert dbl["double"] >= 16 and dbl["order_two"] >= 4 and dbl["inf"] >= 2, dbl
    # the j of y = j p that reach the order-two branch of xyzz_dbl_rho: all that were chosen, up to the end of y's interval
    reached = {c["j"] for c in rm.dbl_cases(name) if c["rung"] == "order_two" and not c["inf"]}
    assert reached == set(rm.dbl_zero_multiples(name)), (name, sorted(reached))
    top = 2 if s.first_needs_reduction(u.nr if u.deg == 2 else 0) else 1 << s.D
    assert {0, 1, -1, 2, -2, top, -top} <= reached and (top < 63 or {63, -63} <= reached), (name, sorted(reached))
    assert all(rm.maybe_zero(s, rm.limbs_of(s, j * s.p), s.K) for j in reached), "inside the filter's promise"
    jac = Counter((c["op"], c["rung"]) for c in rm.jac_cases(name))
    for k in (("madd", "general"), ("madd", "same"), ("madd", "opposite"), ("madd", "first"), ("dbl", "double"), ("dbl", "order_two"),
              ("dbl", "inf"), ("is_inf", "z_zero"), ("is_inf", "finite"), ("is_inf", "flag")):
        assert jac[k] >= 1, (name, k)
    # accumulators at their stated bounds: some value of every state within p of each end of the Checker's interval
    st, _ = rm.states(u.field, u.nr)
    for state in ("first", "steady"):
        xs = [rm.value(s, comp) for c in rm.madd_cases(name) if c["state"] == state and not c["inf"] for comp in c["acc"][0]]
        lo, hi = rm._iv(s, st[state]["x"])
        assert min(xs) - lo < s.p and hi - max(xs) < s.p, (name, state, "x does not reach the ends of its interval")
    ends = [l for c in rm.madd_cases(name) if not c["inf"] for comp in c["acc"][0] for l in comp[:-1]]
    assert min(ends) <= 0 and max(ends) >= s.M, "limbs at the ends of their range"


def _lane_pairs(u, op, args):
    """the (a, b) limb pairs of the scans the device runs for one element, per lane"""
    s, nr = u.s, u.nr
    neg = lambda c: [-l for l in c]
    if op == "mul":
        return [[(args[0][c], args[1][c])] for c in range(u.deg)]
    if op == "sqr":
        return [[(args[0][c], args[0][c])] for c in range(u.deg)]
    if op == "mul2":
        return [[(args[0][c], args[1][c]), (args[2][c], args[3][c])] for c in range(u.deg)]
    k = lambda c: [nr * l for l in c]
    if op == "re_sqr" and nr == -1:   # even lane (x0 + x1)(x0 - x1), odd lane x0 (2 x1); both factors carried where rr_fits(4) fails
        x0, x1 = args[0]
        u, v, w = [a + b for a, b in zip(x0, x1)], [a - b for a, b in zip(x0, x1)], [2 * b for b in x1]
        if not s.fits(4.0):
            return [[(rm.norm(s, u), rm.norm(s, v))], [(rm.norm(s, x0), rm.norm(s, w))]]
        return [[(u, v)], [(x0, w)]]
    x, y = args[0], (args[0] if op == "re_sqr" else args[1])
    lanes = [[(x[0], y[0]), (k(x[1]), y[1])], [(x[0], y[1]), (x[1], y[0])]]
    if op == "re_mul_sub_mul":
        c, d = args[2], args[3]
        lanes[0] += [(neg(c[0]), d[0]), (k(neg(c[1])), d[1])]
        lanes[1] += [(neg(c[0]), d[1]), (neg(c[1]), d[0])]
    return lanes


@pytest.mark.parametrize("fname", rm.FIELDS)
def test_extreme_sets_are_extreme(fname):
    """the worst column of each product's operand set reaches at least half of the Checker's worst_column for factors at
    the invariant 2^B + 8 in every limb (a condition, not a measurement): mul, mul2, sqr, the Fq2 product, the fused
    a b - c d, and the Fq2 square.  NR != -1 (bls12_377): the square is the product x x and is held to the same half.
    NR = -1: the device multiplies u = x0 + x1 by v = x0 - x1, and the Checker bounds u and v as independent factors of
    2 (2^B + 8) per limb, 4 L (2^B + 8)^2 per column.  No operand reaches half of that plus the m p allowance: limb by limb
    |u_i| + |v_i| = 2 max(|x0_i|, |x1_i|) <= 2 (2^B + 8), so the two products u_i v_j + u_j v_i of a column that share
    the limbs i and j are together at most 4 (2^B + 8)^2, and a column at most 2 L (2^B + 8)^2 -- half of the Checker's
    product part alone.  The condition there is that the set reaches this maximum, 2 L (2^B + 8)^2 (sum in the low half of
    the limbs, difference in the high half).  Where both factors are carried first (rr_fits(4) fails: alt_bn128) they are
    ordinary factors of B bits and the half of the Checker's column is asked again."""
    s = rm.shape(fname)
    e = s.fmax
    E = tb.El(-e, e, -e, e, 1.0)

    def worst(name, op, limit=160):
        u = rm.unit(name)
        return max(rm.columns(s, lane) for args in rm.limb_operands(name, op)["args"][:limit] + rm.limb_operands(name, op)["args"][-48:]
                   for lane in _lane_pairs(u, op, args))

    for op, pairs, squares in (("mul", [(E, E)], []), ("mul2", [(E, E), (E, E)], []), ("sqr", [], [E])):
        ch = tb.Checker(s)
        ch.product(pairs, squares=squares)
        got = worst(fname + "_g1", op)
        assert got < 2 ** 63 and 2 * got >= ch.worst_column, (fname, op, got / ch.worst_column)
    if fname in rm.FQ2_NR:
        nr = rm.FQ2_NR[fname]
        mul, _, mul_sub_mul = tb.ops(tb.Checker(s), nr)
        for op in ("re_mul", "re_mul_sub_mul", "re_sqr"):
            if op == "re_mul_sub_mul" and not s.fits(2.0 * (1.0 + abs(nr))):
                continue   # two sums of two and a carry step: the shape of re_mul
            ch = tb.Checker(s)
            m, sq, msm = tb.ops(ch, nr)
            m(E, E) if op == "re_mul" else (sq(E) if op == "re_sqr" else msm(E, E, E, E))
            got = worst(fname + "_g2", op)
            if op == "re_sqr" and nr == -1 and s.fits(4.0):
                assert 2 ** 63 > got >= 2 * s.L * e * e, (fname, op, got / (2 * s.L * e * e))
                continue
            assert got < 2 ** 63 and 2 * got >= ch.worst_column, (fname, op, got / ch.worst_column)


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_381_g2", "bw6_761_g1"])
def test_formulas_agree_with_the_curve(name):
    """the formula-level functions against the curve model of field_model.curve(), on points"""
    import field_model as fm

    u = rm.unit(name)
    F = u.F
    C = fm.curve(name)
    pts = rm._curve_points(u)
    plain = lambda P: None if P is fm.INF else tuple(u.res_words(c) for c in P)
    back = lambda P: tuple(u.words_of(c) for c in P)
    for i in range(8):
        P, Q = pts[i], pts[(i + 3) % len(pts)]
        for Q_ in (Q, P, (P[0], F.sub(F.zero, P[1]))):
            want = plain(C.add(back(P), back(Q_)))
            got, _ = rm.f_madd(F, (P[0], P[1], F.one, F.one), Q_, False)
            aff = None if got is rm.INF else (F.mul(got[0], F.inv(got[2])), F.mul(got[1], F.inv(got[3])))
            assert aff == want
            got, _ = rm.f_add(F, (P[0], P[1], F.one, F.one), (Q_[0], Q_[1], F.one, F.one))
            aff = None if got is rm.INF else (F.mul(got[0], F.inv(got[2])), F.mul(got[1], F.inv(got[3])))
            assert aff == want
            got, _ = rm.f_jac_madd(F, (P[0], P[1], F.one), Q_)
            if got is not rm.INF:
                zi = F.inv(got[2])
                got = (F.mul(got[0], F.sqr(zi)), F.mul(got[1], F.mul(F.sqr(zi), zi)))
            assert got == want
