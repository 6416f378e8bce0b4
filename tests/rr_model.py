"""Plain-integer model of the reduced-radix layer (libff_amd/csrc/rr.cuh): field elements as L signed limbs of B bits,
Montgomery radix rho = 2^(B L), never reduced.  The moduli and non-residues come from tests/field_model.py.

Most functions of the layer have a uniquely determined output, and the model restates them from their CONTRACTS, not from
their column loops:
  * a product scan of S = sum a_j b_j returns exactly (S + m p) / rho with 0 <= m < rho, m = -S p^-1 (mod rho), with limbs
    0 .. L-2 in [0, 2^B) and the sign in the top limb (`dot`, `limbs_of`);
  * rr_ripple returns that same form of its input's value; rr_canon_product the form of value mod p;
  * rr_is_zero_exact says whether the value is j p for the only j a's low limb allows, j in [-2^(B-1), 2^(B-1));
  * rr_maybe_zero<K> looks at the low limb alone: j = a[0] p^-1 (mod 2^B), centred, lies in [-K, K).
So the device is compared limb for limb.  The point functions are compared as residues, coordinate by coordinate, against
the formulas they implement (madd-2008-s, mdbl-2008-s-1, add-2008-s, dbl-2008-s-1, dbl-2009-l, madd-2007-bl), which are
polynomial identities and so hold for operands that are no curve points; operands that are points are also checked
against the curve model of field_model.curve().

The second half builds the operands: field edges as words, factor extremes as limbs, representatives of zero spread
differently over the limbs with their near misses, accumulators at the bounds tests/test_rr_bounds.py derives (taken from
its Checker by import), and the special-case ladder of every point function.
"""
import functools
import math
import random
from fractions import Fraction

import numpy as np

import field_model as fm

FIELDS = ["alt_bn128", "bls12_377", "bls12_381", "bw6_761"]
# the eight units that accumulate on reduced-radix limbs (libff_amd/build.py GROUP_FLAGS: ACC_RR), name -> field
UNITS = {g[0]: g[3] for g in fm.GROUPS if not g[0].startswith("mnt")}
MODULI = {f: (fm.field(f).p, fm.field(f).N) for f in FIELDS}
FQ2_NR = {g[3]: g[5] for g in fm.GROUPS if g[4] == 2 and g[3] in FIELDS}


class Shape:
    """rr_shape<P> of rr.cuh"""

    def __init__(self, name):
        self.name = name
        self.p, self.N = MODULI[name]
        bits = self.bits = self.p.bit_length()
        self.B = 29 if bits + 6 <= 9 * 29 else 28           # rr_shape<P>::B
        self.L = (bits + 6 + self.B - 1) // self.B           # rr_shape<P>::L
        self.D = self.B * self.L - 32 * self.N               # rho = 2^D 2^(32N)
        self.BL = self.B * self.L
        self.rho = 1 << self.BL
        self.ratio = self.p / self.rho                       # p / rho
        self.M = (1 << self.B) - 1
        self.K = (1 << self.D) + 64                          # rr_filter_k<P>
        self.pinv = pow(self.p, -1, 1 << self.B)             # p^-1 mod 2^B
        self.npinv_rho = (-pow(self.p, -1, self.rho)) % self.rho
        self.fmax = (1 << self.B) + 8                        # the factor invariant: |limb| <= 2^B + 8
        assert 0 <= self.D < self.B

    def first_needs_reduction(self, nr):
        return bool(nr) and self.D + 2 >= self.BL - self.bits   # rr_first_needs_reduction

    def fits(self, weighted_products):
        """rr_fits<P>: does a column of that many (weighted) products plus the m p products stay below 2^63"""
        return (weighted_products + 1.0) * float(self.L) * float(self.fmax) * float(self.fmax) < 9.2e18


@functools.lru_cache(maxsize=None)
def shape(name):
    return Shape(name)


# ---- limbs <-> integers --------------------------------------------------------------------------
def value(s, limbs):
    return sum(int(l) << (s.B * i) for i, l in enumerate(limbs))


def limbs_of(s, v):
    """the form a product leaves: limbs 0 .. L-2 in [0, 2^B), the sign in the top limb"""
    out = [(v >> (s.B * i)) & s.M for i in range(s.L - 1)]
    out.append(v >> (s.B * (s.L - 1)))
    return out


def fits_i32(limbs):
    return all(-2 ** 31 <= l < 2 ** 31 for l in limbs)


def respread(s, limbs, positions, sign=1):
    """the same value with 2^B moved between neighbours: limb i + sign 2^B, limb i + 1 - sign"""
    out = list(limbs)
    for i in positions:
        out[i] += sign << s.B
        out[i + 1] -= sign
    return out


# ---- the deterministic functions, from their contracts -------------------------------------------
def dot_value(s, S):
    """(S + m p) / rho with 0 <= m < rho"""
    m = (S * s.npinv_rho) % s.rho
    r, rem = divmod(S + m * s.p, s.rho)
    assert rem == 0
    return r


def dot(s, pairs):
    return limbs_of(s, dot_value(s, sum(value(s, a) * value(s, b) for a, b in pairs)))


def mul(s, a, b):
    return dot(s, [(a, b)])


def mul_pow2(s, a, e):
    assert e < s.BL
    return limbs_of(s, dot_value(s, value(s, a) << e))


def pow2_const(s, e):
    return limbs_of(s, pow(2, e, s.p))


def norm(s, a):
    """one parallel carry step: every limb below the top keeps its low B bits and hands the rest, signed, one up"""
    hi = [l >> s.B for l in a[:-1]]
    return [a[0] & s.M] + [(a[i] & s.M) + hi[i - 1] for i in range(1, s.L - 1)] + [a[-1] + hi[-1]]


def ripple(s, a):
    return limbs_of(s, value(s, a))


def canon_product(s, a):
    v = value(s, a)
    assert -s.p < v < 2 * s.p
    return limbs_of(s, v % s.p)


def canon_side(s, a):
    v = value(s, a)
    return "negative" if v < 0 else ("ge_p" if v >= s.p else "neither")


def from_words(s, w, off=0):
    return limbs_of(s, w << off)


def first_q(s, w):
    """the quotient estimate of rr_first_reduced from the top word (its three lines restated: the estimate is part of the
    function's definition) and the true quotient floor(2^D w / p)"""
    pt1 = (s.p >> (32 * (s.N - 1))) + 1
    sh = 0
    while sh < 31 and ((1 << (32 + sh + 1 + s.D)) // pt1) < (1 << 32):
        sh += 1
    recip = (1 << (32 + sh + s.D)) // pt1
    q = min((((w >> (32 * (s.N - 1))) * recip) >> 32) >> sh, 1 << s.D)
    return q, (w << s.D) // s.p


def first_reduced(s, w):
    q, _ = first_q(s, w)
    return [a - b for a, b in zip(from_words(s, w, s.D), limbs_of(s, q * s.p))]


def first_coord(s, nr, w):
    return first_reduced(s, w) if s.first_needs_reduction(nr) else from_words(s, w, s.D)


def export_value(s, a, sh):
    """rr_export_component<SH>: canonical words of a 2^(32N - SH) / rho"""
    r = dot_value(s, value(s, a) << (32 * s.N - sh))
    assert -s.p < r < 2 * s.p, "operand outside what the export assumes"
    return r % s.p


def is_zero_exact(s, a):
    """a = j p for the one j the low limb allows"""
    v = value(s, a)
    return v % s.p == 0 and -(1 << (s.B - 1)) <= v // s.p < (1 << (s.B - 1))


def maybe_zero(s, a, K):
    j = (a[0] * s.pinv) & s.M
    if j >= 1 << (s.B - 1):
        j -= 1 << s.B
    return -K <= j < K


def small_times(s, a, k):
    return norm(s, [k * l for l in a])


@functools.lru_cache(maxsize=None)
def _zero_j_limit(fname):
    s = shape(fname)
    ok = lambda j: fits_i32(limbs_of(s, j * s.p)) and fits_i32(limbs_of(s, -j * s.p))   # monotone in j: only the top limb grows
    lo, hi = 0, 1 << 40
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return min(lo, (1 << (s.B - 1)) - 1)


def zero_j_limit(s):
    """J: the largest |j| for which j p and -j p, rippled, keep their top limb in int32 and which rr_is_zero_exact's
    signed B-bit j can still name (computed per field, by bisection)"""
    return _zero_j_limit(s.name)


# element-level products: lists of deg components, each a limb list
def el_mul(s, nr, x, y):
    if len(x) == 1:
        return [dot(s, [(x[0], y[0])])]
    nx1 = [nr * l for l in x[1]]
    return [dot(s, [(x[0], y[0]), (nx1, y[1])]), dot(s, [(x[0], y[1]), (x[1], y[0])])]


def el_sqr(s, nr, x):
    """Fq2 with NR = -1: (x0 + x1)(x0 - x1) and x0 (2 x1) -- the same integers S as the product x x, so the same limbs"""
    return el_mul(s, nr, x, x)


def el_mul_sub_mul(s, nr, a, b, c, d):
    if len(a) == 1:
        return [dot(s, [(a[0], b[0]), ([-l for l in c[0]], d[0])])]
    if s.fits(2.0 * (1.0 + abs(nr))):   # one fused sum of four products per lane
        V = lambda e: [value(s, k) for k in e]
        a_, b_, c_, d_ = V(a), V(b), V(c), V(d)
        s0 = a_[0] * b_[0] + nr * a_[1] * b_[1] - c_[0] * d_[0] - nr * c_[1] * d_[1]
        s1 = a_[0] * b_[1] + a_[1] * b_[0] - c_[0] * d_[1] - c_[1] * d_[0]
        return [limbs_of(s, dot_value(s, s0)), limbs_of(s, dot_value(s, s1))]
    u, v = el_mul(s, nr, a, b), el_mul(s, nr, c, d)   # two sums of two and a carry step
    return [norm(s, [p - q for p, q in zip(u[k], v[k])]) for k in range(2)]


def columns(s, pairs):
    """largest |column sum| the scan of sum a_j b_j holds before its shift (the m p products included): what must stay
    below 2^63"""
    S = sum(value(s, a) * value(s, b) for a, b in pairs)
    m = limbs_of(s, (S * s.npinv_rho) % s.rho)
    pl = limbs_of(s, s.p)
    acc, worst = 0, 0
    for k in range(2 * s.L - 1):
        lo, hi = max(0, k - s.L + 1), min(k, s.L - 1)
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        acc += sum(m[i] * pl[k - i] for i in range(lo, hi + 1))
        worst = max(worst, abs(acc))
        acc >>= s.B
    return worst


# ---- residues: Fq / Fq2 on plain integers ----------------------------------------------------------
class Res:
    """the coordinate field of a unit on plain residues (no Montgomery factor): tuples of deg integers mod p"""

    def __init__(self, p, deg, nr):
        self.p, self.deg, self.nr = p, deg, nr
        self.zero = (0,) * deg
        self.one = (1,) + (0,) * (deg - 1)

    def mul(self, a, b):
        p = self.p
        if self.deg == 1:
            return (a[0] * b[0] % p,)
        return ((a[0] * b[0] + self.nr * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def k(self, k, a):
        return tuple(k * x % self.p for x in a)

    def sqr(self, a):
        return self.mul(a, a)

    def inv(self, a):
        p = self.p
        if self.deg == 1:
            return (pow(a[0], -1, p),)
        t = pow((a[0] * a[0] - self.nr * a[1] * a[1]) % p, -1, p)
        return (a[0] * t % p, -a[1] * t % p)


class Unit:
    def __init__(self, name):
        _, self.curve, self.group, self.field, self.deg, self.nr = fm.GROUP_BY_NAME[name]
        self.name = name
        self.s = shape(self.field)
        self.F = Res(self.s.p, self.deg, self.nr)
        s = self.s
        self.inv_rho = pow(s.rho, -1, s.p)
        self.inv_rho_d = pow(s.rho << s.D, -1, s.p)
        self.inv_r = pow(1 << (32 * s.N), -1, s.p)

    # residues of elements given as limbs / words
    def res(self, el, factor="rho"):
        f = self.inv_rho if factor == "rho" else self.inv_rho_d
        return tuple(value(self.s, c) * f % self.s.p for c in el)

    def res_words(self, ws):
        return tuple(w * self.inv_r % self.s.p for w in ws)

    def words_of(self, r):
        """canonical Montgomery words (factor 2^(32N)) of a residue"""
        return tuple((c << (32 * self.s.N)) % self.s.p for c in r)


@functools.lru_cache(maxsize=None)
def unit(name):
    return Unit(name)


INF = None


def f_madd(F, acc, pt, neg):
    """madd-2008-s with the ladder of xyzz_madd_rr on residues.  acc: (X, Y, ZZ, ZZZ) or INF, pt: (x, y), (0, 0) =
    infinity.  -> (result or INF, rung)"""
    x2, y2 = pt
    if x2 == F.zero and y2 == F.zero:
        return acc, "point_inf"
    if neg:
        y2 = F.sub(F.zero, y2)
    if acc is INF:
        return (x2, y2, F.one, F.one), "first"
    X, Y, ZZ, ZZZ = acc
    P = F.sub(F.mul(x2, ZZ), X)
    R = F.sub(F.mul(y2, ZZZ), Y)
    if P == F.zero:
        if R != F.zero:
            return INF, "opposite"
        if pt[1] == F.zero:
            return INF, "order_two"
        V = F.k(4, F.sqr(y2))
        W = F.k(2, F.mul(y2, V))
        S = F.mul(x2, V)
        M = F.k(3, F.sqr(x2))
        X3 = F.sub(F.sqr(M), F.k(2, S))
        return (X3, F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, y2)), V, W), "same"
    PP = F.sqr(P)
    PPP = F.mul(P, PP)
    Q = F.mul(X, PP)
    X3 = F.sub(F.sub(F.sqr(R), PPP), F.k(2, Q))
    return (X3, F.sub(F.mul(R, F.sub(Q, X3)), F.mul(Y, PPP)), F.mul(ZZ, PP), F.mul(ZZZ, PPP)), "general"


def f_dbl(F, a):
    """dbl-2008-s-1 (a = 0) with the order-two branch of xyzz_dbl_rho"""
    if a is INF:
        return INF, "inf"
    X, Y, ZZ, ZZZ = a
    if Y == F.zero:
        return INF, "order_two"
    U = F.k(2, Y)
    V = F.sqr(U)
    W = F.mul(U, V)
    S = F.mul(X, V)
    M = F.k(3, F.sqr(X))
    X3 = F.sub(F.sqr(M), F.k(2, S))
    return (X3, F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, Y)), F.mul(V, ZZ), F.mul(W, ZZZ)), "double"


def f_add(F, a, b):
    """add-2008-s with the ladder of xyzz_add_rho"""
    if b is INF:
        return a, "b_inf"
    if a is INF:
        return b, "a_inf"
    X1, Y1, ZZ1, ZZZ1 = a
    X2, Y2, ZZ2, ZZZ2 = b
    U1, S1 = F.mul(X1, ZZ2), F.mul(Y1, ZZZ2)
    P = F.sub(F.mul(X2, ZZ1), U1)
    R = F.sub(F.mul(Y2, ZZZ1), S1)
    if P == F.zero:
        if R != F.zero:
            return INF, "opposite"
        r, rung = f_dbl(F, a)
        return r, "equal" if rung == "double" else "equal_order_two"
    PP = F.sqr(P)
    PPP = F.mul(P, PP)
    Q = F.mul(U1, PP)
    X3 = F.sub(F.sub(F.sqr(R), PPP), F.k(2, Q))
    return (X3, F.sub(F.mul(R, F.sub(Q, X3)), F.mul(S1, PPP)), F.mul(F.mul(ZZ1, ZZ2), PP),
            F.mul(F.mul(ZZZ1, ZZZ2), PPP)), "general"


def f_jac_dbl(F, a):
    """dbl-2009-l (a = 0) with the order-two branch of jac_dbl_rr"""
    if a is INF:
        return INF, "inf"
    X, Y, Z = a
    if Y == F.zero:
        return INF, "order_two"
    A, B = F.sqr(X), F.sqr(Y)
    C = F.sqr(B)
    Dd = F.k(2, F.sub(F.sub(F.sqr(F.add(X, B)), A), C))
    E = F.k(3, A)
    X3 = F.sub(F.sqr(E), F.k(2, Dd))
    return (X3, F.sub(F.mul(E, F.sub(Dd, X3)), F.k(8, C)), F.k(2, F.mul(Y, Z))), "double"


def f_jac_madd(F, a, pt):
    """madd-2007-bl with the ladder of jac_madd_rr"""
    px, py = pt
    if a is INF:
        return (px, py, F.one), "first"
    X, Y, Z = a
    ZZ = F.sqr(Z)
    H = F.sub(F.mul(px, ZZ), X)
    r = F.sub(F.mul(py, F.mul(Z, ZZ)), Y)
    if H == F.zero:
        if r != F.zero:
            return INF, "opposite"
        res, rung = f_jac_dbl(F, (px, py, F.one))
        return res, "same" if rung == "double" else "same_order_two"
    HH = F.sqr(H)
    I = F.k(4, HH)
    J = F.mul(H, I)
    r = F.k(2, r)
    V = F.mul(X, I)
    X3 = F.sub(F.sub(F.sqr(r), J), F.k(2, V))
    return (X3, F.sub(F.mul(r, F.sub(V, X3)), F.k(2, F.mul(Y, J))), F.k(2, F.mul(Z, H))), "general"


# ---- operand builders ------------------------------------------------------------------------------
def _dedup(seq):
    seen, out = set(), []
    for v in seq:
        k = tuple(v) if isinstance(v, (list, tuple)) else v
        if k not in seen:
            seen.add(k)
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def word_edges(fname):
    """field edges as words in [0, p): the small and large values, 2^k - 1, every limb boundary 2^(B k) and its
    neighbours, the 32-bit edges of field_model"""
    s = shape(fname)
    p = s.p
    raw = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    raw += [(1 << k) - 1 for k in range(1, s.bits)]
    for k in range(1, s.L):
        raw += [(1 << (s.B * k)) - 1, 1 << (s.B * k), (1 << (s.B * k)) + 1]
        raw += [(1 << (s.B * k - s.D)) + d for d in (-1, 0, 1) if s.B * k - s.D > 0]   # boundaries after the shift by D
    raw += fm.edges(fname)
    return _dedup(v for v in raw if 0 <= v < p)


@functools.lru_cache(maxsize=None)
def first_words(fname, seed=5):
    """words for rr_first_reduced: the edges, random values, and by search values whose top-word estimate is exact and
    values where it is one short (w just above a multiple of p / 2^D: the estimate rounds the top word down)"""
    s = shape(fname)
    rng = random.Random(f"{fname}/first/{seed}")
    out = list(word_edges(fname)) + [rng.randrange(s.p) for _ in range(256)]
    for q in list(range(1, min(1 << s.D, 24))) + [(1 << s.D) - 1 - k for k in range(min(1 << s.D, 8))]:
        if not 0 < q < (1 << s.D):
            continue
        w0 = -(-(q * s.p) >> s.D)   # the least w with floor(2^D w / p) = q
        out += [w for w in (w0 - 1, w0, w0 + 1, w0 + rng.randrange(1 << 20)) if 0 <= w < s.p]
    return _dedup(out)


def first_sides(s, words):
    exact = sum(1 for w in words if first_q(s, w)[0] == first_q(s, w)[1])
    short = sum(1 for w in words if first_q(s, w)[0] + 1 == first_q(s, w)[1])
    assert exact + short == len(words), "the estimate is never too large and at most one too small"
    return {"exact": exact, "one_short": short}


def _rand_factor(s, rng):
    """limbs anywhere inside the factor invariant"""
    return [rng.randrange(-s.fmax, s.fmax + 1) for _ in range(s.L)]


@functools.lru_cache(maxsize=None)
def factor_extremes(fname):
    """limb vectors at the factor invariant |limb| <= 2^B + 8: all +, all -, alternating, one extreme limb at each
    position, the top limb at the invariant too"""
    s = shape(fname)
    e = s.fmax
    out = [[e] * s.L, [-e] * s.L, [e if i % 2 == 0 else -e for i in range(s.L)], [-e if i % 2 == 0 else e for i in range(s.L)]]
    for i in range(s.L):
        for sg in (1, -1):
            out.append([sg * e if j == i else 0 for j in range(s.L)])
            out.append([sg * e if j == i else (j * 7919 + 1) & s.M for j in range(s.L)])
    return out


@functools.lru_cache(maxsize=None)
def product_operands(fname, arity, n_random=384, seed=3):
    """operand tuples (arity limb vectors each) for the per-component products: every pair of extremes, the sign patterns
    that align every product of a column (b reversed against a, so that a[i] b[k - i] all carry one sign), canonical
    values, random factors"""
    s = shape(fname)
    rng = random.Random(f"{fname}/prod/{arity}/{seed}")
    ext = factor_extremes(fname)
    e = s.fmax
    alt = [e if i % 2 == 0 else -e for i in range(s.L)]
    # a[i] b[k - i] > 0 for every i in column k = L - 1: b[j] takes the sign of a[L - 1 - j]
    aligned = []
    for a in ([e] * s.L, [-e] * s.L, alt):
        b = [e if a[s.L - 1 - j] > 0 else -e for j in range(s.L)]
        aligned += [(a, b), (a, [-l for l in b])]
    canon = [limbs_of(s, w) for w in word_edges(fname)[:48]]
    out = []
    if arity == 1:
        out = [(a,) for a in ext + canon]
    elif arity == 2:
        out = aligned + [(a, b) for a in ext[:6] for b in ext] + [(a, b) for a in canon[:12] for b in canon[:12]]
    else:   # a b + c d: both products of every column with one sign (the 3 L (2^B + 8)^2 case), and with opposite signs
        for a, b in aligned:
            out += [(a, b, a, b), (a, b, [-l for l in a], b), (a, b, b, a)]
        out += [(a, b, c, d) for a in ext[:4] for b in ext[:4] for c in ext[:4] for d in ext[:4]]
    while len(out) < n_random + 64:
        out.append(tuple(_rand_factor(s, rng) for _ in range(arity)))
    return out


def lift(unit_, comps, rng_seed=1):
    """per-component operand tuples -> elements of the unit: for an Fq2 unit the given value in one component and
    another operand of the list in the other"""
    if unit_.deg == 1:
        return [tuple([c] for c in cs) for cs in comps]
    rng = random.Random(f"{unit_.name}/lift/{rng_seed}")
    out = []
    for k, cs in enumerate(comps):
        other = comps[rng.randrange(len(comps))]
        out.append(tuple([c, o] if k % 2 == 0 else [o, c] for c, o in zip(cs, other)))
    out += [tuple([c, c] for c in cs) for cs in comps[:32]]
    # NR < 0: with x = (a, -a), y = (b, b) the even lane's a b + (NR x1) y1 is (1 + |NR|) a b -- where a b aligns every
    # product of a column (the first tuples of product_operands), so does the fused sum; likewise a b - c d with c = (-c, c)
    neg = lambda c: [-l for l in c]
    for cs in comps[:48]:
        if len(cs) == 2:
            out.append(([cs[0], neg(cs[0])], [cs[1], cs[1]]))
        elif len(cs) == 4:
            out.append(([cs[0], neg(cs[0])], [cs[1], cs[1]], [neg(cs[2]), cs[2]], [cs[3], cs[3]]))
    return out


@functools.lru_cache(maxsize=None)
def zero_reps(fname):
    """representatives of zero and their near misses.  -> list of (limbs, j or None, kind): kind 'zero' (value j p),
    'miss' (a near miss: j p +- 1, +- 2^B, +- 2^(B (L - 1))) or 'low_limb' (j p + 2^B t: the low limb of j p, so the
    filter passes and only the exact test can reject it)"""
    s = shape(fname)
    J = zero_j_limit(s)
    js = [0]
    for K in (64, s.K):
        js += [K - 1, K, K + 1]
    js = _dedup([0, 1, 2] + js + [J])
    js = _dedup([j for j in js if j <= J] + [-j for j in js if 0 < j <= J])
    out = []
    pos = _dedup([0, 1, s.L // 2, s.L - 2])
    for j in js:
        base = limbs_of(s, j * s.p)
        forms = [base] + [respread(s, base, [i], sg) for i in pos for sg in (1, -1)]
        forms.append(respread(s, base, list(range(0, s.L - 1, 2)), -1))   # negative low limbs all the way up
        forms.append(respread(s, base, list(range(s.L - 1)), 1))
        for f in forms:
            if fits_i32(f):
                out.append((f, j, "zero"))
        for d in (1, -1, 1 << s.B, -(1 << s.B), 1 << (s.B * (s.L - 1)), -(1 << (s.B * (s.L - 1)))):
            f = limbs_of(s, j * s.p + d)
            if fits_i32(f):
                out.append((f, j, "miss"))
                out.append((respread(s, f, [0], 1), j, "miss"))
        for t in (1, 12345, -7):
            f = limbs_of(s, j * s.p + (t << s.B))
            if fits_i32(f):
                out.append((f, j, "low_limb"))
    return out


def filter_sides(s, K, reps):
    """pass with exact zero / pass without (a false positive) / no pass, and the false negatives (must be none: |j| < K)"""
    cnt = {"pass_zero": 0, "pass_nonzero": 0, "no_pass": 0, "false_negative": 0}
    for f, j, kind in reps:
        m, z = maybe_zero(s, f, K), is_zero_exact(s, f)
        if kind == "zero" and abs(j) < K and not m:
            cnt["false_negative"] += 1
        cnt["pass_zero" if m and z else ("pass_nonzero" if m else "no_pass")] += 1
    return cnt


# ---- accumulator states, with the bounds of tests/test_rr_bounds.py ------------------------------
def _bounds():
    import test_rr_bounds as tb
    return tb


@functools.lru_cache(maxsize=None)
def states(fname, nr):
    """{state: {coordinate: El}} as the Checker of test_rr_bounds.py derives them: 'first' (xyzz_rr_first), 'steady'
    (any number of general additions behind it), 'record' (a record brought to the factor rho: the copied record of the
    general addition), 'sum' (sums of records), and the Checker that walked them"""
    tb = _bounds()
    ch = tb.Checker(shape(fname))
    first = tb.first_point(ch, nr)
    steady = tb.run_sequences(ch, nr)
    recs = []
    for start in (tb.first_point(ch, nr), tb.doubling_path(ch, nr)):
        acc = start
        for _ in range(5):
            recs.append(tb.rec_to_rho(ch, acc))
            acc = tb.madd(ch, acc, fq2_nr=nr)
    recs.append(tb.canonical_to_rho(ch, nr))
    record = recs[0]
    for r in recs[1:]:
        record = tb.widen(record, r)
    return {"first": first, "steady": steady, "record": record, "sum": tb.general_add_states(ch, nr)}, ch


def _iv(s, el):
    """the Checker's value interval in integers (its ends are floats in units of p)"""
    return math.ceil(Fraction(el.vlo) * s.p), math.floor(Fraction(el.vhi) * s.p)


def rep_in(s, el, rng, mode):
    """limbs of one representative inside the Checker's interval `el`, of whatever residue: 'rippled' (limbs 0 .. L-2 in
    [0, 2^B)) or 'ends' (each of those limbs at an end of its range, at most [-4, 2^B + 4)); the value near the low end,
    near the high end or anywhere inside"""
    top_w = s.B * (s.L - 1)
    vlo, vhi = _iv(s, el)
    where = rng.randrange(3)
    v = vlo + rng.randrange(1 << 64) if where == 0 else (vhi - rng.randrange(1 << 64) if where == 1 else rng.randrange(vlo, vhi + 1))
    v = min(max(v, vlo), vhi)
    if mode == "ends":
        lo, hi = max(el.lo, -4), min(el.hi, (1 << s.B) + 3)
        low = [rng.choice((lo, hi)) for _ in range(s.L - 1)]
        out = low + [min(max((v - value(s, low + [0])) >> top_w, el.tlo), el.thi)]
        if vlo <= value(s, out) <= vhi:
            return out
    out = limbs_of(s, v)
    assert el.tlo <= out[-1] <= el.thi, (el, out[-1])
    return out


def in_interval(s, el, limbs):
    """None when limbs and value lie inside the Checker's interval, else what does not"""
    if not all(el.lo <= l <= el.hi for l in limbs[:-1]):
        return f"limb outside [{el.lo}, {el.hi}]"
    if not el.tlo <= limbs[-1] <= el.thi:
        return f"top limb {limbs[-1]} outside [{el.tlo}, {el.thi}]"
    v = value(s, limbs)
    vlo, vhi = _iv(s, el)   # exact: the interval's ends are floats, their products with p are taken as rationals
    if not vlo <= v <= vhi:
        return f"value {v / s.p:.3f} p outside [{el.vlo:.3f}, {el.vhi:.3f}] p"
    return None


def el_with_residue(u, el, res_c, rng):
    """limbs of the residue res_c (an integer mod p, already carrying its Montgomery factor) inside the interval: res + k p
    with k at an end of the interval or inside, rippled.  -> (limbs, k)"""
    s = u.s
    vlo, vhi = _iv(s, el)
    kmin, kmax = -((res_c - vlo) // s.p), (vhi - res_c) // s.p
    assert kmin <= kmax, (el, "no representative of the residue inside the interval")
    k = rng.choice((kmin, kmax, rng.randint(kmin, kmax)))
    return limbs_of(s, res_c + k * s.p), k


# ---- point cases -------------------------------------------------------------------------------------
def _rand_res(u, rng, nonzero=True):
    return tuple(rng.randrange(1 if nonzero else 0, u.s.p) for _ in range(u.deg))


def _curve_points(u):
    """affine points of the unit's curve as plain residues"""
    C = fm.curve(u.name)
    pts = [C.add(C.base[j % 16], C.base[(5 * j + 3) % 16]) for j in range(16)] + list(C.base)
    return [tuple(u.res_words(c) for c in P) for P in pts if P is not fm.INF]


def _limbs_el(u, el_iv, res, factor, rng, mode):
    """element (deg limb lists) of residue res (plain) with the factor 'rho' / 'rho_d' inside the interval el_iv"""
    s = u.s
    f = s.rho if factor == "rho" else s.rho << s.D
    out = []
    for c in res:
        limbs, _ = el_with_residue(u, el_iv, c * f % s.p, rng)
        if mode == "ends":   # move 2^B between neighbours where the range allows it, keeping the value
            lo, hi = max(el_iv.lo, -4), min(el_iv.hi, (1 << s.B) + 3)
            for i in range(s.L - 2):
                if limbs[i] + (1 << s.B) <= hi and limbs[i + 1] - 1 >= lo and rng.randrange(2):
                    limbs = respread(s, limbs, [i], 1)
                elif limbs[i] - (1 << s.B) >= lo and limbs[i + 1] + 1 <= hi and rng.randrange(2):
                    limbs = respread(s, limbs, [i], -1)
        out.append(limbs)
    return out


def _free_el(u, el_iv, rng, mode):
    """an element inside the interval of whatever residue (formula-level operands need not be points)"""
    return [rep_in(u.s, el_iv, rng, mode) for _ in range(u.deg)]


def _one_el(u, e):
    """the element (2^e mod p, 0) as re_set_pow2 builds it"""
    return [pow2_const(u.s, e)] + [[0] * u.s.L for _ in range(u.deg - 1)]


@functools.lru_cache(maxsize=None)
def madd_cases(name, seed=7):
    """the ladder of xyzz_madd_rr.  -> list of dicts: acc (4 elements of limbs), inf, pt (2 tuples of words), neg, want
    (residue quadruple or INF), rung, state, zz_factor"""
    u = unit(name)
    s, F = u.s, u.F
    st, _ = states(u.field, u.nr)
    rng = random.Random(f"{name}/madd/{seed}")
    pts = _curve_points(u)
    cases = []

    def acc_of(quad, state, mode):
        iv = st[state]
        return [_limbs_el(u, iv[k], quad[i], "rho" if k in ("x", "y") else "rho_d", rng, mode)
                for i, k in enumerate(("x", "y", "zz", "zzz"))]

    def push(quad, state, mode, pt, neg, inf=False, acc=None):
        acc = acc if acc is not None else acc_of(quad, state, mode)
        got = tuple(u.res(acc[i], "rho" if i < 2 else "rho_d") for i in range(4))
        want, rung = f_madd(F, INF if inf else got, pt, neg)
        if want is INF and rung == "point_inf" and inf:
            want = INF
        cases.append(dict(acc=acc, inf=inf, pt=tuple(u.words_of(c) for c in pt), neg=neg, want=want, rung=rung, state=state))

    def scaled(P, z):
        zz = F.sqr(z)
        zzz = F.mul(zz, z)
        return (F.mul(P[0], zz), F.mul(P[1], zzz), zz, zzz)

    negate = lambda P: (P[0], F.sub(F.zero, P[1]))
    for k in range(96):   # general addition: arbitrary residues (formula level) and curve points, both states, both spreads
        state, mode = ("steady", "first")[k % 2], ("rippled", "ends")[(k // 2) % 2]
        if k % 3 == 0:
            P, Q = pts[k % len(pts)], pts[(k + 5) % len(pts)]
            quad = scaled(P, _rand_res(u, rng)) if state == "steady" else (P[0], P[1], F.one, F.one)
            push(quad, state, mode, Q, bool(k & 4))
        else:   # formula level: limbs anywhere inside the state's intervals (mode 'ends': at the ends of the limb range)
            iv = st[state]
            one = _one_el(u, s.BL + s.D)
            acc = [_free_el(u, iv["x"], rng, mode), _free_el(u, iv["y"], rng, mode)]
            acc += [one, one] if state == "first" else [_free_el(u, iv["zz"], rng, mode), _free_el(u, iv["zzz"], rng, mode)]
            push(None, state, mode, (_rand_res(u, rng), _rand_res(u, rng)), bool(k & 4), acc=acc)
    zero_acc = [[[0] * s.L for _ in range(u.deg)] for _ in range(4)]
    for k in range(16):   # first point into an empty accumulator (whatever limbs the accumulator holds), (0, 0) as the point
        P = pts[k % len(pts)] if k % 2 else (_rand_res(u, rng), _rand_res(u, rng))
        push(None, "first", "rippled", P, bool(k & 2), inf=True, acc=zero_acc if k % 4 < 2 else acc_of(tuple(_rand_res(u, rng) for _ in range(4)), "steady", "rippled"))
        push(tuple(_rand_res(u, rng) for _ in range(4)), "steady", "rippled", (F.zero, F.zero), bool(k & 2))
    push(None, "first", "rippled", (F.zero, F.zero), False, inf=True, acc=zero_acc)
    # x close to p: the first point is x 2^D as an integer, so P = U2 - X1 = j p with |j| near 2^D
    near_p = [tuple((s.p - 1 - rng.randrange(1 << 16)) for _ in range(u.deg)) for _ in range(8)]
    for k in range(48):   # same point / opposite point, directly after a first point and on a steady accumulator
        state, mode = ("first", "steady")[k % 2], ("rippled", "ends")[(k // 2) % 2]
        if k % 4 == 0:   # words near p (not a curve point: the ladder decides on x and y alone)
            P = (u.res_words(near_p[k % 8]), _rand_res(u, rng))
        else:
            P = pts[k % len(pts)]
        neg_pt = bool(k & 8)
        # acc holds +-P in the sense the device will see after its own negation
        held = P if (k // 16) % 2 == 0 else negate(P)          # same / opposite
        shown = negate(P) if neg_pt else P                      # the words given; neg turns them back into P
        quad = scaled(held, _rand_res(u, rng)) if state == "steady" else (held[0], held[1], F.one, F.one)
        acc = None
        if state == "first" and k % 4 == 0:   # the accumulator exactly as xyzz_rr_first leaves it: x 2^D as an integer
            nr = u.nr if u.deg == 2 else 0
            fx = [first_coord(s, nr, w) for w in u.words_of(held[0])]
            if s.first_needs_reduction(nr):
                fx = [norm(s, c) for c in fx]
            one = _one_el(u, s.BL + s.D)
            acc = [fx, [norm(s, first_coord(s, nr, w)) for w in u.words_of(held[1])], one, one]
        push(quad, state, mode, shown, neg_pt, acc=acc)
    for k in range(8):    # y = 0 in words: the order-two branch (same x, R = 0, y = 0)
        x = _rand_res(u, rng)
        state = ("first", "steady")[k % 2]
        quad = scaled((x, F.zero), _rand_res(u, rng)) if state == "steady" else (x, F.zero, F.one, F.one)
        push(quad, state, "rippled", (x, F.zero), bool(k & 2))
    return cases


@functools.lru_cache(maxsize=None)
def add_cases(name, seed=9):
    """the ladder of xyzz_add_rho and xyzz_dbl_rho, every coordinate with the factor rho.  -> list of dicts: a, b (4
    elements of limbs), a_inf, b_inf, want, rung"""
    u = unit(name)
    s, F = u.s, u.F
    st, _ = states(u.field, u.nr)
    rng = random.Random(f"{name}/add/{seed}")
    pts = _curve_points(u)
    cases = []

    def rec(quad, state, mode):
        iv = st[state]
        return [_limbs_el(u, iv[k], quad[i], "rho", rng, mode) for i, k in enumerate(("x", "y", "zz", "zzz"))]

    def scaled(P, z):
        zz = F.sqr(z)
        zzz = F.mul(zz, z)
        return (F.mul(P[0], zz), F.mul(P[1], zzz), zz, zzz)

    def push(a, b, sa_, sb_, a_inf=False, b_inf=False):
        ra = INF if a_inf else tuple(u.res(e) for e in a)
        rb = INF if b_inf else tuple(u.res(e) for e in b)
        want, rung = f_add(F, ra, rb)
        cases.append(dict(a=a, b=b, a_inf=a_inf, b_inf=b_inf, want=want, rung=rung, sa=sa_, sb=sb_))

    negate = lambda P: (P[0], F.sub(F.zero, P[1]))
    rq = lambda: tuple(_rand_res(u, rng) for _ in range(4))
    sa = ("record", "sum")
    for k in range(64):
        mode = ("rippled", "ends")[k % 2]
        A, Bs = sa[(k // 2) % 2], sa[(k // 4) % 2]
        if k % 3 == 0:
            P, Q = pts[k % len(pts)], pts[(k + 3) % len(pts)]
            push(rec(scaled(P, _rand_res(u, rng)), A, mode), rec(scaled(Q, _rand_res(u, rng)), Bs, mode), A, Bs)
        else:   # formula level
            free = lambda state: [_free_el(u, st[state][c], rng, mode) for c in ("x", "y", "zz", "zzz")]
            push(free(A), free(Bs), A, Bs)
    for k in range(32):   # equal sums, opposite sums: a first-point record (ZZ = ZZZ = 1) on either side or scaled ones
        P = pts[k % len(pts)] if k % 4 else (_rand_res(u, rng), _rand_res(u, rng))
        Q = P if k % 2 == 0 else negate(P)
        mode = ("rippled", "ends")[(k // 4) % 2]
        qa = (P[0], P[1], F.one, F.one) if (k // 4) % 3 == 0 else scaled(P, _rand_res(u, rng))
        qb = (Q[0], Q[1], F.one, F.one) if (k // 4) % 3 == 1 else scaled(Q, _rand_res(u, rng))
        push(rec(qa, sa[(k // 2) % 2], mode), rec(qb, sa[(k // 8) % 2], mode), sa[(k // 2) % 2], sa[(k // 8) % 2])
    for k in range(8):    # infinity on each side, both; equal points of order two
        push(rec(rq(), "sum", "rippled"), rec(rq(), "record", "rippled"), "sum", "record", a_inf=bool(k & 1), b_inf=bool(k & 2))
    for k in range(4):
        x = _rand_res(u, rng)
        push(rec(scaled((x, F.zero), _rand_res(u, rng)), "sum", "rippled"), rec(scaled((x, F.zero), _rand_res(u, rng)), "record", "rippled"), "sum", "record")
    return cases


@functools.lru_cache(maxsize=None)
def dbl_cases(name, seed=10):
    """xyzz_dbl_rho: records and sums; y = 0 given in limbs as j p (the order-two branch), for j over the filter's range"""
    u = unit(name)
    s, F = u.s, u.F
    st, _ = states(u.field, u.nr)
    rng = random.Random(f"{name}/dbl/{seed}")
    cases = []
    js = dbl_zero_multiples(name)
    for k in range(48):
        state, mode = ("record", "sum")[k % 2], ("rippled", "ends")[(k // 2) % 2]
        iv = st[state]
        a = [_free_el(u, iv[c], rng, mode) for c in ("x", "y", "zz", "zzz")]
        inf = k % 16 == 14
        j = None
        if k % 4 == 3:   # y = j p in limbs: the order-two branch; twelve slots for at most nine values of j
            j = js[(k // 4) % len(js)]
            a[1] = [limbs_of(s, j * s.p) for _ in range(u.deg)]
        ra = INF if inf else tuple(u.res(e) for e in a)
        want, rung = f_dbl(F, ra)
        cases.append(dict(a=a, inf=inf, want=want, rung=rung, state=state, j=j))
    return cases


def dbl_zero_multiples(name):
    """the j with y = j p given to xyzz_dbl_rho: 0, +-1, +-2, +-63 where the Checker's interval of a record's or a sum's
    y holds them, and the ends of that interval, +-2^D where the first point is not reduced ("y of a record copied into the
    sum may still be a first point's") -- a y outside the interval is no input of the function; the filter's own K - 1 =
    2^D + 63 lies outside it"""
    u = unit(name)
    st, _ = states(u.field, u.nr)
    lo = min(st[k]["y"].vlo for k in ("record", "sum"))
    hi = max(st[k]["y"].vhi for k in ("record", "sum"))
    return [j for j in _dedup([0, 1, -1, 2, -2, 63, -63, math.floor(hi), math.ceil(lo)]) if abs(j) <= 2 or lo <= j <= hi]


@functools.lru_cache(maxsize=None)
def jac_cases(name, seed=11):
    """jac_dbl_rr, jac_madd_rr, jac_is_inf_rr: X, Y, Z with the factor rho in the form re_from_words_rho leaves (a
    product's output, value in (0, 2p)) or after a step; affine operand likewise.  -> list of dicts"""
    u = unit(name)
    s, F = u.s, u.F
    rng = random.Random(f"{name}/jac/{seed}")
    pts = _curve_points(u)
    cases = []

    def prod_form(res, k=None):
        out = []
        for c in res:
            v = c * s.rho % s.p
            out.append(limbs_of(s, v + (rng.randrange(2) if k is None else k) * s.p))
        return out

    def jac(P, z):
        zz = F.sqr(z)
        return (F.mul(P[0], zz), F.mul(P[1], F.mul(zz, z)), z)

    negate = lambda P: (P[0], F.sub(F.zero, P[1]))
    for k in range(40):
        P, Q = pts[k % len(pts)], pts[(k + 7) % len(pts)]
        z = F.one if k % 5 == 0 else _rand_res(u, rng)
        kind = ("general", "same", "opposite", "first", "formula")[k % 5] if k >= 10 else "general"
        inf = kind == "first"
        if kind == "same":
            Q = P
        elif kind == "opposite":
            Q = negate(P)
        a = jac(P, z) if kind != "formula" else tuple(_rand_res(u, rng) for _ in range(3))
        if kind == "formula":
            Q = (_rand_res(u, rng), _rand_res(u, rng))
        al = [prod_form(c) for c in a]
        ql = [prod_form(c) for c in Q]
        ra = INF if inf else tuple(u.res(e) for e in al)
        want, rung = f_jac_madd(F, ra, tuple(u.res(e) for e in ql))
        cases.append(dict(op="madd", a=al, q=ql, inf=inf, want=want, rung=rung))
        wd, rd = f_jac_dbl(F, ra)
        cases.append(dict(op="dbl", a=al, q=None, inf=inf, want=wd, rung=rd))
    for j in (0, 1, -1, 2, 63, -63):   # y = 0 in limbs as j p: doubling to infinity; Z = j p: jac_is_inf_rr
        a = [prod_form(_rand_res(u, rng)) for _ in range(3)]
        a[1] = [limbs_of(s, j * s.p) for _ in range(u.deg)]
        cases.append(dict(op="dbl", a=a, q=None, inf=False, want=INF, rung="order_two"))
        b = [prod_form(_rand_res(u, rng)) for _ in range(3)]
        b[2] = [limbs_of(s, j * s.p) for _ in range(u.deg)]
        cases.append(dict(op="is_inf", a=b, q=None, inf=False, want=True, rung="z_zero"))
        cases.append(dict(op="is_inf", a=a, q=None, inf=False, want=False, rung="finite"))
    cases.append(dict(op="is_inf", a=[prod_form(_rand_res(u, rng)) for _ in range(3)], q=None, inf=True, want=True, rung="flag"))
    return cases


# ---- arrays ------------------------------------------------------------------------------------------
def limb_rows(els):
    """list of elements (deg limb lists each) -> (n * deg, L) int32"""
    a = np.array([c for e in els for c in e], dtype=np.int64)
    assert a.size == 0 or (a.min() >= -2 ** 31 and a.max() < 2 ** 31), "a limb outside int32"
    return a.astype(np.int32)


def word_rows(s, vals):
    """list of tuples of deg integers -> (n * deg, N) uint32"""
    buf = b"".join(int(c).to_bytes(4 * s.N, "little") for e in vals for c in e)
    return np.frombuffer(buf, dtype="<u4").reshape(-1, s.N).copy()


def words_value(row):
    return int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little")


def quad_rows(recs, deg):
    """list of records (4 elements of deg limb lists) -> (n * deg, 4 L) int32: row = one component's x, y, zz, zzz"""
    a = np.array([[l for e in r for l in e[c]] for r in recs for c in range(deg)], dtype=np.int64)
    assert a.size == 0 or (a.min() >= -2 ** 31 and a.max() < 2 ** 31), "a limb outside int32"
    return a.astype(np.int32)


def quad_of_rows(s, rows, deg, i):
    """record i of an (n * deg, 4 L) array -> 4 elements of deg limb lists"""
    return [[[int(v) for v in rows[i * deg + c, k * s.L:(k + 1) * s.L]] for c in range(deg)] for k in range(4)]


# ---- the limb-level probe: operands and expected results per op ---------------------------------------
# op codes of Engine.rr_probe (include/amdmsm.h amdmsm_rr_probe_device); small_times_k: op 18 with k
ROPS = {"mul": 0, "mul2": 1, "sqr": 2, "re_mul": 3, "re_sqr": 4, "re_mul_sub_mul": 5, "mul_pow2_32n": 6, "mul_pow2_32n_d": 7,
        "from_words_rho": 8, "export_0": 9, "export_d": 10, "norm": 16, "ripple": 17, "small_times_2": 18, "small_times_3": 18,
        "small_times_4": 18, "cneg": 19, "from_words_0": 20, "from_words_d": 21, "first_reduced": 22, "first_coord": 23,
        "to_words": 24, "canon_product": 25, "is_zero_exact": 26, "maybe_zero_k": 27, "maybe_zero_64": 28, "set_pow2_bl": 29,
        "set_pow2_bl_d": 30}
REDUCED_LIST = ["mul", "sqr", "re_mul", "re_sqr", "is_zero_exact", "maybe_zero_k", "maybe_zero_64"]   # bw6_761_g2
XOPS = {"madd": 0, "first": 1, "rec_to_rho": 2, "export": 3, "export_rho": 4, "dbl_rho": 8, "add_rho": 9, "jac_dbl": 16,
        "jac_madd": 17, "jac_is_inf": 18}
WORD_OPS = ("from_words_rho", "from_words_0", "from_words_d", "first_reduced", "first_coord")
I32_SAFE = 2 ** 31 - 16   # limbs of this magnitude survive one carry from below without leaving int32


def unit_ops(name):
    """the ops a unit runs: everything, less first_reduced where the table of multiples is not built (D > 8), and the
    reduced list for bw6_761_g2"""
    if name == "bw6_761_g2":
        return list(REDUCED_LIST)
    return [op for op in ROPS if op != "first_reduced" or unit(name).s.D <= 8]


def _wide_limbs(s, bound, rng, n_random=192):
    """limb vectors up to `bound` in magnitude: all at the bound with either sign, alternating, one at each position, a top
    limb at the bound over canonical limbs, random"""
    out = [[bound] * s.L, [-bound] * s.L, [bound if i % 2 == 0 else -bound for i in range(s.L)],
           [-bound if i % 2 == 0 else bound for i in range(s.L)]]
    for i in range(s.L):
        for sg in (1, -1):
            out.append([sg * bound if j == i else 0 for j in range(s.L)])
            out.append([sg * bound if j == i else rng.randrange(-bound, bound + 1) for j in range(s.L)])
    out += [[rng.randrange(-bound, bound + 1) for _ in range(s.L)] for _ in range(n_random)]
    out += [[rng.randrange(s.M + 1) for _ in range(s.L - 1)] + [sg * bound] for sg in (1, -1)]
    return out


@functools.lru_cache(maxsize=None)
def export_operands(fname, sh, seed=4):
    """components as a record holds them, for rr_export_component<SH>: residues plus k p over |value| < 2^(D + SH) p (where
    a 2^(32N - SH) / rho lies in (-p, 2p): what the export assumes), as far as int32 limbs reach, rippled and with 2^B moved
    between limbs; and the values -c 2^(D + SH) and p + c 2^(D + SH), which the reduction sends to -c and to p + c exactly
    (m = 0, and m = rho - 2^(32N - SH)): the negative and the >= p side of rr_canon_product with small operands"""
    s = shape(fname)
    rng = random.Random(f"{fname}/export/{sh}/{seed}")
    kmax = min((1 << (s.D + sh)) - 1, zero_j_limit(s) - 1)
    kk = _dedup([0, 1, -1, 2, -2, kmax - 1, -kmax, kmax // 2, -(kmax // 2)])
    out = []
    for c in range(1, 25):
        out += [limbs_of(s, -(c << (s.D + sh))), limbs_of(s, s.p + (c << (s.D + sh)))]
    for r in word_edges(fname)[:40] + [rng.randrange(s.p) for _ in range(96)]:
        for k in (kk if len(out) < 400 else [rng.choice(kk)]):
            base = limbs_of(s, r + k * s.p)
            out.append(base)
            i = rng.randrange(s.L - 1)
            out.append(respread(s, base, [i], rng.choice((1, -1))))
    return out


def _fit_tops(name, op, args):
    """a product leaves its sign and everything above B (L - 1) bits in the top limb, an int32: where factors with every
    limb at the invariant would push a fused sum past that (the top limbs alone decide it), the operands' top limbs are
    halved until the result fits -- the largest top limbs the function's output form allows, within a factor of two"""
    while True:
        out, _, _ = limb_expected(name, op, args)
        if all(fits_i32(c) for c in out):
            return args
        args = tuple([c[:-1] + [c[-1] // 2 if c[-1] > 0 else -((-c[-1]) // 2)] for c in e] for e in args)


@functools.lru_cache(maxsize=None)
def limb_operands(name, op):
    """-> dict: 'args' (list of operand tuples: elements of deg limb lists, or of deg words for the word ops), 'k'"""
    u = unit(name)
    s, f = u.s, u.field
    rng = random.Random(f"{name}/{op}")
    k = int(op[-1]) if op.startswith("small_times") else 0
    if op in ("mul", "re_mul"):
        args = lift(u, product_operands(f, 2))
    elif op in ("mul2", "re_mul_sub_mul"):
        args = lift(u, product_operands(f, 4))
    elif op in ("sqr", "re_sqr"):
        args = lift(u, product_operands(f, 1))
        if op == "re_sqr" and u.deg == 2:
            e, h = s.fmax, s.L // 2
            alt = [e if i % 2 == 0 else -e for i in range(s.L)]
            args += [
                # NR != -1 (the square is the product x x): x0[i] x0[k - i] > 0 and x1[i] x1[k - i] < 0 in every odd
                # column, so x0 x0 + (NR x1) x1 aligns all (1 + |NR|) L products of column L - 1 (L is even there)
                ([[e] * s.L, alt],), ([[-e] * s.L, alt],),
                # NR = -1, (x0 + x1)(x0 - x1): the sum at 2 (2^B + 8) in the low half of the limbs, the difference in the
                # high half -- column L - 1 then holds L / 2 products of 4 (2^B + 8)^2, the most any operand reaches
                ([[e] * s.L, [e] * h + [-e] * (s.L - h)],), ([[e] * s.L, [-e] * h + [e] * (s.L - h)],),
                # ... and where both factors are carried first (rr_fits(4) fails): limbs that survive the carry step
                ([[s.M] * s.L, [0] * s.L],), ([[0] * s.L, [s.M] * s.L],),
            ]
    elif op in ("mul_pow2_32n", "mul_pow2_32n_d"):
        args = lift(u, product_operands(f, 1) + [(a,) for a in _wide_limbs(s, I32_SAFE, rng, 64)])
    elif op in ("export_0", "export_d"):
        args = lift(u, [(a,) for a in export_operands(f, 0 if op == "export_0" else s.D)])
    elif op in ("norm", "ripple"):
        args = lift(u, [(a,) for a in _wide_limbs(s, I32_SAFE, rng) + factor_extremes(f)])
    elif op.startswith("small_times"):
        # k a must stay in int32 and leave the top limb room for a carry; [2^B - 1] * L: 4 (2^29 - 1) = 2^31 - 4, a product's
        # output at its largest, times four
        bound = min(s.fmax, I32_SAFE // k)
        args = lift(u, [(a,) for a in _wide_limbs(s, I32_SAFE // k, rng) + _wide_limbs(s, bound, rng, 16)
                        + [[s.M] * (s.L - 1) + [I32_SAFE // k]]])
    elif op == "cneg":
        args = lift(u, [(a,) for a in _wide_limbs(s, 2 ** 31 - 1, rng)])
    elif op in ("from_words_rho", "from_words_0", "from_words_d"):
        ws = word_edges(f) + [rng.randrange(s.p) for _ in range(256)]
        args = [(tuple(ws[(i + 17 * c) % len(ws)] for c in range(u.deg)),) for i in range(len(ws))]
    elif op in ("first_reduced", "first_coord"):
        ws = first_words(f)
        args = [(tuple(ws[(i + 17 * c) % len(ws)] for c in range(u.deg)),) for i in range(len(ws))]
    elif op == "to_words":
        args = lift(u, [(limbs_of(s, w),) for w in word_edges(f) + [rng.randrange(s.p) for _ in range(256)]])
    elif op == "canon_product":
        p = s.p
        vs = [-p + 1, -p + 2, -1, 0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p - 2]
        vs += [w + d for w in word_edges(f)[:64] for d in (-p, 0, p) if -p < w + d < 2 * p]
        vs += [rng.randrange(-p + 1, 2 * p) for _ in range(256)]
        args = lift(u, [(limbs_of(s, v),) for v in _dedup(vs)])
    elif op in ("is_zero_exact", "maybe_zero_k", "maybe_zero_64"):
        reps = [r[0] for r in zero_reps(f)]
        comps = [(a,) for a in reps] + [(_rand_factor(s, rng),) for _ in range(64)]
        if u.deg == 1:
            args = [([a],) for (a,) in comps]
        else:   # a zero in both components (any two representatives), in one only, in neither
            zs = [r[0] for r in zero_reps(f) if r[2] == "zero"]
            args = [([a, zs[(7 * i) % len(zs)]],) for i, (a,) in enumerate(comps)]
            args += [([zs[(5 * i) % len(zs)], a],) for i, (a,) in enumerate(comps)]
            args += [([a, reps[(3 * i + 1) % len(reps)]],) for i, (a,) in enumerate(comps)]
    elif op in ("set_pow2_bl", "set_pow2_bl_d"):
        args = [([[0] * s.L] * u.deg,) for _ in range(65)]
    else:
        raise ValueError(op)
    if op in ("mul", "mul2", "sqr", "re_mul", "re_sqr", "re_mul_sub_mul"):
        args = [_fit_tops(name, op, a) for a in args]
    if len(args) % 2 == 0 and op in ("mul", "norm", "is_zero_exact", "from_words_d"):
        args = args[:-1]   # an odd count
    return dict(args=args, k=k)


def limb_expected(name, op, args):
    """-> (out element or None, out words tuple or None, flag) for one operand tuple"""
    u = unit(name)
    s, nr = u.s, u.nr
    comp = lambda fn: [fn(*[e[c] for e in args]) for c in range(u.deg)]
    if op == "mul":
        return comp(lambda a, b: mul(s, a, b)), None, 0
    if op == "mul2":
        return comp(lambda a, b, c, d: dot(s, [(a, b), (c, d)])), None, 0
    if op == "sqr":
        return comp(lambda a: mul(s, a, a)), None, 0
    if op == "re_mul":
        return el_mul(s, nr, *args), None, 0
    if op == "re_sqr":
        return el_sqr(s, nr, args[0]), None, 0
    if op == "re_mul_sub_mul":
        return el_mul_sub_mul(s, nr, *args), None, 0
    if op == "mul_pow2_32n":
        return comp(lambda a: mul_pow2(s, a, 32 * s.N)), None, 0
    if op == "mul_pow2_32n_d":
        return comp(lambda a: mul_pow2(s, a, 32 * s.N - s.D)), None, 0
    if op == "from_words_rho":
        c = pow2_const(s, s.BL + s.D)
        return [mul(s, from_words(s, w), c) for w in args[0]], None, 0
    if op in ("export_0", "export_d"):
        return args[0], tuple(export_value(s, a, 0 if op == "export_0" else s.D) for a in args[0]), 0
    if op == "norm":
        return comp(lambda a: norm(s, a)), None, 0
    if op == "ripple":
        return comp(lambda a: ripple(s, a)), None, 0
    if op.startswith("small_times"):
        return comp(lambda a: small_times(s, a, int(op[-1]))), None, 0
    if op == "from_words_0":
        return [from_words(s, w) for w in args[0]], None, 0
    if op == "from_words_d":
        return [from_words(s, w, s.D) for w in args[0]], None, 0
    if op == "first_reduced":
        return [first_reduced(s, w) for w in args[0]], None, 0
    if op == "first_coord":
        return [first_coord(s, nr if u.deg == 2 else 0, w) for w in args[0]], None, 0
    if op == "to_words":
        return args[0], tuple(value(s, a) for a in args[0]), 0
    if op == "canon_product":
        return comp(lambda a: canon_product(s, a)), None, 0
    if op == "is_zero_exact":
        return args[0], None, int(all(is_zero_exact(s, a) for a in args[0]))
    if op in ("maybe_zero_k", "maybe_zero_64"):
        K = s.K if op == "maybe_zero_k" else 64
        return args[0], None, int(all(maybe_zero(s, a, K) for a in args[0]))
    if op in ("set_pow2_bl", "set_pow2_bl_d"):
        return _one_el(u, s.BL if op == "set_pow2_bl" else s.BL + s.D), None, 0
    raise ValueError(op)


def cneg_expected(args_list):
    """rr_cneg negates the elements of odd index"""
    return [[[-l for l in c] for c in a[0]] if i % 2 else a[0] for i, a in enumerate(args_list)]


def factor_limit(name, op):
    """the largest limb magnitude the callee allows its operands: the factor invariant for the products, int32 otherwise"""
    s = unit(name).s
    if op in ("mul", "mul2", "sqr", "re_mul", "re_sqr", "re_mul_sub_mul"):
        return s.fmax
    return 2 ** 31 - 1


def madd_same_x_multiple(name, case):
    """j per component with P = U2 - X1 = j p for a same-x case of xyzz_madd_rr (U2 as the device computes it: the product
    of the point's words and ZZ); None where P is no multiple of p"""
    u = unit(name)
    s = u.s
    px = [from_words(s, w) for w in case["pt"][0]]
    u2 = el_mul(s, u.nr, px, case["acc"][2])
    out = []
    for c in range(u.deg):
        v = value(s, u2[c]) - value(s, case["acc"][0][c])
        if v % s.p:
            return None
        out.append(v // s.p)
    return out
