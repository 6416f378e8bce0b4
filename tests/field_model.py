"""Plain-integer model of the coordinate fields of all eleven groups, as the device stores them: Fq and
Fq2 = Fq[u]/(u^2 - NR) in Montgomery form with R = 2^(32 N), N = the field's 32-bit words.  Independent of the
oracle: the moduli come from tests/golden/golden.npz and tests/mnt_model.py, everything else is derived here.

Beside the exact results the model computes the unreduced quantities the device corrects -- t of a Montgomery
product, the unreduced column sum of a fused sum of products with the factor representatives the device builds
(2p - x, 10p - 5x, 5x), the sign of a - b, the sum a + b -- so that a test can count, on the CPU, which side of each
data-dependent correction an operand takes.

The second half generates the operand sets of tests/test_field_model_cpu.py and tests/test_gpu_field_probe.py:
operands are chosen as STORED words (the carry chains see the stored bits), deterministically per field.
"""
import functools
import os
import random
from fractions import Fraction

import numpy as np

import mnt_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))

# name, curve id, group id, field name, extension degree, non-residue
GROUPS = [
    ("alt_bn128_g1", 0, 1, "alt_bn128", 1, 0), ("alt_bn128_g2", 0, 2, "alt_bn128", 2, -1),
    ("bls12_377_g1", 1, 1, "bls12_377", 1, 0), ("bls12_377_g2", 1, 2, "bls12_377", 2, -5),
    ("bw6_761_g1", 2, 1, "bw6_761", 1, 0), ("bw6_761_g2", 2, 2, "bw6_761", 1, 0),
    ("bls12_381_g1", 3, 1, "bls12_381", 1, 0), ("bls12_381_g2", 3, 2, "bls12_381", 2, -1),
    ("mnt4_g1", 4, 1, "mnt4", 1, 0), ("mnt4_g2", 4, 2, "mnt4", 2, 17), ("mnt6_g1", 5, 1, "mnt6", 1, 0),
]
GROUP_BY_NAME = {g[0]: g for g in GROUPS}
FIELD_NAMES = ["alt_bn128", "bls12_377", "bw6_761", "bls12_381", "mnt4", "mnt6"]
# element types whose cold kernels are built fully inlined (libff_amd/build.py AMDMSM_COLD_INLINE): impl 0 == impl 1
COLD_INLINE = {"alt_bn128_g1", "bls12_377_g1", "bls12_381_g1", "mnt4_g1", "mnt6_g1"}

# op codes of Engine.field_probe (include/amdmsm.h)
OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "neg": 4, "inv": 5, "dbl": 6, "cneg": 7, "half": 8, "to_mont": 9,
       "from_mont": 10, "sqrt": 11, "mul_lz": 16, "sqr_lz": 17, "sub_lz": 18, "add_lz": 19, "neg_lz": 20,
       "mul_sub_mul_lz": 21, "is_zero_lz": 22, "canon": 23}
CANONICAL_OPS = ["mul", "sqr", "add", "sub", "neg", "inv", "dbl", "cneg", "half", "to_mont", "from_mont", "sqrt"]
LAZY_OPS = ["mul_lz", "sqr_lz", "sub_lz", "add_lz", "neg_lz", "mul_sub_mul_lz", "is_zero_lz", "canon"]
ARITY = {"mul": 2, "add": 2, "sub": 2, "cneg": 2, "mul_lz": 2, "sub_lz": 2, "add_lz": 2, "mul_sub_mul_lz": 4}


class Field:
    """Fq in Montgomery form, R = 2^(32 N); every method works on stored integers"""

    def __init__(self, name, p, n_words):
        self.name, self.p, self.N = name, p, n_words
        self.bits = p.bit_length()
        self.R = 1 << (32 * n_words)
        self.Rinv = pow(self.R, -1, p)
        self.npinv = (-pow(p, -1, self.R)) % self.R   # -p^-1 mod R
        self.r1, self.r2 = self.R % p, self.R * self.R % p
        self.top = p >> (32 * (n_words - 1))          # top 32-bit limb
        assert 4 * p <= self.R

    # ---- unreduced quantities
    def dot_t(self, xs, ys):
        """(sum x_j y_j + m p) / R with m = -(sum) p^-1 mod R: what the column scan holds before any correction"""
        s = sum(x * y for x, y in zip(xs, ys))
        m = (s * self.npinv) & (self.R - 1)
        return (s + m * self.p) >> (32 * self.N)

    def mont_t(self, a, b):
        return self.dot_t((a,), (b,))

    def dot_subs(self, T, F2=4):
        """fp_dot_subs of fp.cuh: conditional subtractions of 2p after a fused sum of T products whose factor
        bounds multiply to at most F2 p^2, from the bound (T F2 (top + 1) / 2^32 + 1) p"""
        bound = Fraction(T * F2 * (self.top + 1), 1 << 32) + 1
        if bound <= 2:
            return 0
        n, b = 0, bound
        while b > 2:
            b = b - 2 if b - 2 > 2 else Fraction(2)
            n += 1
            if b <= 2:
                break
        return n

    def dot_reduce(self, t, nsubs):
        """-> (value, [whether subtraction k of 2p fired])"""
        fired = []
        for _ in range(nsubs):
            f = t >= 2 * self.p
            fired.append(f)
            if f:
                t -= 2 * self.p
        return t, fired

    # ---- factor representatives of the fused sums (fp.cuh / fp2.cuh)
    def neg_lz(self, x):
        return 0 if x in (0, self.p) else 2 * self.p - x

    def nr_factor(self, nr, x):
        return 2 * self.p - x if nr == -1 else 10 * self.p - 5 * x

    # ---- exact results on stored values
    def mul(self, a, b):
        return a * b * self.Rinv % self.p

    def inv(self, a):
        return pow(a, -1, self.p) * self.r2 % self.p

    def is_square(self, a):
        a %= self.p
        return a == 0 or pow(a, (self.p - 1) // 2, self.p) == 1


class Ext:
    """the coordinate field of one group: Fq (deg 1) or Fq2; elements are tuples of deg stored integers"""

    def __init__(self, F, deg, nr):
        self.F, self.deg, self.nr = F, deg, nr

    def mul(self, a, b):
        F, p = self.F, self.F.p
        if self.deg == 1:
            return (F.mul(a[0], b[0]),)
        return ((a[0] * b[0] + self.nr * a[1] * b[1]) * F.Rinv % p, (a[0] * b[1] + a[1] * b[0]) * F.Rinv % p)

    def add(self, a, b):
        return tuple((x + y) % self.F.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.F.p for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % self.F.p for x in a)

    def half(self, a):
        h = (self.F.p + 1) // 2
        return tuple(x * h % self.F.p for x in a)

    def one(self):
        return (self.F.r1,) + (0,) * (self.deg - 1)

    def zero(self):
        return (0,) * self.deg

    def small(self, k):
        return (k * self.F.r1 % self.F.p,) + (0,) * (self.deg - 1)

    def inv(self, a):
        F, p = self.F, self.F.p
        if self.deg == 1:
            return (F.inv(a[0]),)
        norm = (F.mul(a[0], a[0]) - self.nr * F.mul(a[1], a[1])) % p
        t = F.inv(norm)
        return (F.mul(a[0], t), -F.mul(a[1], t) % p)

    def norm(self, a):
        F = self.F
        return a[0] % F.p if self.deg == 1 else (F.mul(a[0], a[0]) - self.nr * F.mul(a[1], a[1])) % F.p

    def is_square(self, a):
        """Fq2: a^((p^2 - 1) / 2) = norm(a)^((p - 1) / 2); R is a square, so stored and plain values agree"""
        return self.F.is_square(self.norm(a))

    # ---- the fused sums the inline element types run (fp2.cuh), as lists of (xs, ys, T, F2)
    def fused(self):
        """inline types only: Fq always, Fq2 for NR < 0 (NR = 17 runs Karatsuba)"""
        return self.deg == 1 or self.nr < 0

    def mul_lz_sums(self, x, y):
        if self.deg == 1 or not self.fused():
            return []
        F, f2 = self.F, (4 if self.nr == -1 else 20)
        return [((x[0], F.nr_factor(self.nr, x[1])), (y[0], y[1]), 2, f2), ((x[0], x[1]), (y[1], y[0]), 2, 4)]

    def mul_sub_mul_lz_sums(self, a, b, c, d):
        F, p = self.F, self.F.p
        if self.deg == 1:
            return [((a[0], F.neg_lz(c[0])), (b[0], d[0]), 2, 4)]
        if not self.fused():
            return []
        f2 = 4 if self.nr == -1 else 20
        pc1 = c[1] if self.nr == -1 else 5 * c[1]
        return [((a[0], F.nr_factor(self.nr, a[1]), 2 * p - c[0], pc1), (b[0], b[1], d[0], d[1]), 4, f2),
                ((a[0], a[1], 2 * p - c[0], 2 * p - c[1]), (b[1], b[0], d[1], d[0]), 4, 4)]


def _golden():
    return np.load(os.path.join(HERE, "golden", "golden.npz"))


@functools.lru_cache(maxsize=None)
def field(name):
    if name in ("mnt4", "mnt6"):
        return Field(name, mm.CURVES[name].p, 2 * mm.WORDS)
    limbs = _golden()[f"{name}_g1/fq_modulus"]
    return Field(name, sum(int(w) << (64 * i) for i, w in enumerate(limbs)), 2 * len(limbs))


@functools.lru_cache(maxsize=None)
def ext(group_name):
    _, _, _, fname, deg, nr = GROUP_BY_NAME[group_name]
    return Ext(field(fname), deg, nr)


# ---- words <-> integers ------------------------------------------------------------------------
def to_words(F, elems):
    """list of tuples of stored integers -> (n, deg * N / 2) uint64"""
    nb = 4 * F.N
    buf = b"".join(c.to_bytes(nb, "little") for e in elems for c in e)
    deg = len(elems[0]) if elems else 1
    return np.frombuffer(buf, dtype="<u8").reshape(len(elems), deg * F.N // 2).copy()


def from_words(F, arr, deg):
    nb = 4 * F.N
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    row = nb * deg
    return [tuple(int.from_bytes(raw[i * row + k * nb:i * row + (k + 1) * nb], "little") for k in range(deg))
            for i in range(arr.shape[0])]


# ---- operand sets ------------------------------------------------------------------------------
def _dedup(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def edges(fname, lazy=False):
    """the edge values of the field, clipped to [0, p) or, lazy, [0, 2p)"""
    F = field(fname)
    p, N = F.p, F.N
    ones = lambda k: (1 << (32 * k)) - 1
    raw = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.r1, F.r2, p - F.r1]
    for k in range(1, N + 1):
        raw += [ones(k), 1 << (32 * k), (1 << (32 * k)) + 1]
    for k in range(1, N):   # the largest value below p whose low k limbs are all ones
        v = ((p >> (32 * k)) << (32 * k)) | ones(k)
        raw.append(v if v < p else v - (1 << (32 * k)))
    for k in range(N):      # p with one limb forced to 0 / to all ones
        raw += [p & ~(0xffffffff << (32 * k)), p | (0xffffffff << (32 * k))]
    alt = sum(0xffffffff << (64 * k) for k in range((N + 1) // 2))
    for pat in (alt, alt << 32):
        raw += [pat & ones(N), pat & ((1 << (F.bits - 1)) - 1)]
    raw += [1 << (F.bits - 1), (1 << (F.bits - 1)) - 1]
    canon = _dedup(v for v in raw if 0 <= v < p)
    if not lazy:
        return canon
    return _dedup(canon + [v for v in raw if p <= v < 2 * p] + [p, p + 1, 2 * p - 1, 2 * p - 2] + [p + v for v in canon])


def boundary_pairs(fname, count=128, seed=11):
    """canonical pairs whose Montgomery product has t >= p: a b = y R (mod p) with y < p^2 / 4R and a, b >= p / 2, so
    a b / R > y and t, which is y mod p and above a b / R, is y + p"""
    F = field(fname)
    rng, p, out = random.Random(seed), F.p, []
    while len(out) < count:
        y = rng.randrange(1, p * p // (4 * F.R))
        a = rng.randrange((p + 1) // 2, p)
        b = y * F.R * pow(a, -1, p) % p
        if 2 * b >= p:
            assert F.mont_t(a, b) == y + p
            out.append((a, b))
    return out


def _sqrt_mod(a, p):
    """Tonelli-Shanks on plain integers; None for a non-residue"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) == 1:
        z += 1
    c, x, b, m = pow(z, t, p), pow(a, (t + 1) // 2, p), pow(a, t, p), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % p, i + 1
        w = pow(c, 1 << (m - i - 1), p)
        x, c, b, m = x * w % p, w * w % p, b * w * w % p, i
    return x


def boundary_squares(fname, count=64, seed=12):
    """canonical a >= p / 2 with a^2 = y R (mod p), y < p^2 / 4R: t = y + p as in boundary_pairs"""
    F = field(fname)
    rng, p, out = random.Random(seed), F.p, []
    while len(out) < count:
        y = rng.randrange(1, p * p // (4 * F.R))
        a = _sqrt_mod(y * F.R, p)
        if a is None:
            continue
        a = max(a, p - a)
        assert F.mont_t(a, a) == y + p
        out.append(a)
    return out


def _lift(E, rng, comps_list, pool):
    """Fq operand tuples -> elements of E: the given value in component 0 or 1, a pool value in the other"""
    if E.deg == 1:
        return [tuple((c,) for c in cs) for cs in comps_list]
    out = []
    for k, cs in enumerate(comps_list):
        oth = [pool[rng.randrange(len(pool))] for _ in cs]
        out.append(tuple((c, o) if k % 2 == 0 else (o, c) for c, o in zip(cs, oth)))
    return out


N_RANDOM = 4096
N_SLOW = 512


@functools.lru_cache(maxsize=None)
def operands(group_name, op):
    """-> list of operand tuples (1, 2 or 4 elements of the group's coordinate field, as stored integers)"""
    gname, _, _, fname, deg, nr = GROUP_BY_NAME[group_name]
    E, F = ext(group_name), field(fname)
    p = F.p
    lazy = op in LAZY_OPS
    bound = 2 * p if lazy else p
    rng = random.Random(f"{fname}/{deg}/{op}")
    pool = edges(fname, lazy)
    rnd_el = lambda: tuple(rng.randrange(bound) for _ in range(deg))
    ar = ARITY.get(op, 1)
    if op in ("inv", "sqrt"):
        base = [1, p - 1, F.r1, 2, p - 2, (p - 1) // 2, F.r2] + ([0] if op == "sqrt" else [])
        els = _lift(E, rng, [(v,) for v in base], pool)
        if deg == 2:   # elements of the base field and pure multiples of u, both roots of the complex method
            els += [((v, 0),) for v in base] + [((0, v),) for v in base if v]
        els += _lift(E, rng, [(v,) for v in pool[:96]], pool)
        sq = []
        while len(sq) < 128:   # squares for certain
            x = rnd_el()
            sq.append((E.mul(x, x),))
        els = [e for e in els + sq if op == "sqrt" or any(e[0])]
        while len(els) < N_SLOW:
            els.append((rnd_el(),))
        return els[:N_SLOW]
    if ar == 1:
        comps = [(v,) for v in pool]
        if op in ("sqr", "sqr_lz"):
            comps += [(a,) for a in boundary_squares(fname)]
        import itertools
        zeros = [(e,) for e in itertools.product(*[[v for v in (0, p, 1, p - 1) if v < bound]] * deg)]   # zero is 0 or p
        return _lift(E, rng, comps, pool) + zeros + [(rnd_el(),) for _ in range(N_RANDOM)]
    if ar == 2:
        comps = [(a, b) for a in pool for b in pool]
        if op in ("mul", "mul_lz"):
            comps += boundary_pairs(fname)
        return _lift(E, rng, comps, pool) + [(rnd_el(), rnd_el()) for _ in range(N_RANDOM)]
    # four operands: a b - c d
    pick = lambda: tuple(pool[rng.randrange(len(pool))] for _ in range(deg))
    quads = [(pick(), pick(), pick(), pick()) for _ in range(N_RANDOM)]
    for _ in range(256):
        a, b = pick(), pick()
        quads += [(a, b, a, b), (a, b, b, a), (a, b, E.zero(), pick()), (a, b, pick(), E.zero())]
    # the maximum of the fused sum: every factor at 2p - 1 or 2p - 2 ...
    top = (2 * p - 1, 2 * p - 2)
    for k in range(1 << min(8, 4 * deg)):
        cs = [top[(k >> i) & 1] for i in range(4 * deg)]
        quads.append(tuple(tuple(cs[j * deg:(j + 1) * deg]) for j in range(4)))
    # ... and around it: factors within 8 of 2p - 1; the components the device negates (2p - x, 10p - 5x)
    # within 8 of zero, where the negated factor is largest
    hi = lambda: 2 * p - 1 - rng.randrange(8)
    lo = lambda: rng.randrange(8)
    for k in range(4096):
        if deg == 1:
            quads.append(((hi(),), (hi(),), (lo() + 1,), (hi(),)))
        elif k % 2:   # component 0 of the result: a0 b0 + (NR a1) b1 - c0 d0 - (NR c1) d1
            quads.append(((hi(), lo()), (hi(), hi()), (lo(), hi()), (hi(), hi())))
        else:         # component 1: a0 b1 + a1 b0 - c0 d1 - c1 d0
            quads.append(((hi(), hi()), (hi(), hi()), (lo(), lo()), (hi(), hi())))
    quads += [(rnd_el(), rnd_el(), rnd_el(), rnd_el()) for _ in range(N_RANDOM)]
    return quads


# ---- expected results and checks ---------------------------------------------------------------
def exact(E, op, args):
    """the exact result of a value-returning op on stored operands, canonical per component"""
    F, p = E.F, E.F.p
    a = args[0]
    if op in ("mul", "mul_lz"):
        return E.mul(a, args[1])
    if op in ("sqr", "sqr_lz"):
        return E.mul(a, a)
    if op in ("add", "add_lz"):
        return E.add(a, args[1])
    if op in ("sub", "sub_lz"):
        return E.sub(a, args[1])
    if op in ("neg", "neg_lz"):
        return E.neg(a)
    if op == "inv":
        return E.inv(a)
    if op == "dbl":
        return E.add(a, a)
    if op == "cneg":
        return E.neg(a) if args[1][0] & 1 else a
    if op == "half":
        return E.half(a)
    if op == "to_mont":
        return tuple(x * F.R % p for x in a)
    if op == "from_mont":
        return tuple(x * F.Rinv % p for x in a)
    if op == "mul_sub_mul_lz":
        return E.sub(E.mul(a, args[1]), E.mul(args[2], args[3]))
    if op in ("canon", "is_zero_lz"):
        return tuple(x % p for x in a)
    raise ValueError(op)


def check(E, op, args, out, flag):
    """None when the device's (out, flag) is right for these operands, else a description"""
    F, p = E.F, E.F.p
    if op == "sqrt":
        want = E.is_square(args[0])
        if bool(flag) != want:
            return f"flag {flag}, square: {want}"
        if want and (any(x >= p for x in out) or E.mul(out, out) != args[0]):
            return "out^2 != a"
        return None
    if op == "is_zero_lz":
        want = all(x % p == 0 for x in args[0])
        return None if bool(flag) == want else f"flag {flag}, zero: {want}"
    want = exact(E, op, args)
    if op in LAZY_OPS and op != "canon":
        if any(x >= 2 * p for x in out):
            return "component not below 2p"
        return None if tuple(x % p for x in out) == want else "wrong residue"
    return None if tuple(out) == want else "differs"


# ---- which side of each data-dependent correction an operand set takes -------------------------
def sides(group_name, op, inline=True):
    """{correction: [operands on the 'no correction' side, operands on the 'correction' side]} counted per Fq
    component event, from the model alone.  inline: the element type is fully inlined (fused sums)."""
    E = ext(group_name)
    F, p = E.F, E.F.p
    cnt = {}

    def hit(key, side):
        cnt.setdefault(key, [0, 0])[1 if side else 0] += 1

    for args in operands(group_name, op):
        if op in ("mul", "sqr") and E.deg == 1:
            b = args[1] if op == "mul" else args[0]
            hit("mul t >= p", F.mont_t(args[0][0], b[0]) >= p)
        elif op in ("add", "dbl"):
            b = args[1] if op == "add" else args[0]
            for x, y in zip(args[0], b):
                hit("add a + b >= p", x + y >= p)
        elif op == "sub":
            for x, y in zip(args[0], args[1]):
                hit("sub a < b", x < y)
        elif op == "add_lz":
            for x, y in zip(args[0], args[1]):
                hit("add_lz a + b >= 2p", x + y >= 2 * p)
        elif op == "sub_lz":
            for x, y in zip(args[0], args[1]):
                hit("sub_lz a < b", x < y)
        elif op == "canon":
            for x in args[0]:
                hit("canon a >= p", x >= p)
        elif op == "half":
            for x in args[0]:
                hit("half a odd", x & 1)
        elif op in ("mul_lz", "mul_sub_mul_lz") and inline:
            sums = E.mul_lz_sums(*args) if op == "mul_lz" else E.mul_sub_mul_lz_sums(*args)
            for xs, ys, T, f2 in sums:
                n = F.dot_subs(T, f2)
                t = F.dot_t(xs, ys)
                assert t < (Fraction(T * f2 * (F.top + 1), 1 << 32) + 1) * p and t < F.R
                key = f"dot T={T} max t/p"
                cnt[key] = max(cnt.get(key, 0), t * 1000 // p / 1000)
                v, fired = F.dot_reduce(t, n)
                assert v < 2 * p, (group_name, op, "the model's own reduction left", v / p)
                for k, f in enumerate(fired):
                    hit(f"dot T={T} F2={f2} subtraction {k + 1} of {n}", f)
    return cnt


# ---- the curves, for the point-level probe ----------------------------------------------------
XOPS = {"madd_lz": 0, "madd": 1, "add": 2, "dbl": 3, "dbl_affine": 4, "to_jac": 5}
INF = None


class CurveModel:
    """y^2 = x^3 + a x + b over a group's coordinate field, affine points as pairs of stored elements"""

    def __init__(self, group_name):
        self.name = group_name
        self.E = E = ext(group_name)
        F = E.F
        if group_name.startswith("mnt"):
            c = mm.CURVES[{"mnt4_g1": "mnt4", "mnt4_g2": "mnt4_g2", "mnt6_g1": "mnt6"}[group_name]]
            st = lambda v: tuple(c.fq_mont(x) for x in c.F.comps(v))
            self.a = st(c.a if E.deg == 2 else c.F.c(c.a))
            self.b = st(c.b if E.deg == 2 else c.F.c(c.b))
            self.base = [(st(P[0]), st(P[1])) for P in c.random_points(16, seed=21)]
        else:
            g = _golden()
            self.a = E.zero()
            self.b = from_words(F, g[f"{group_name}/coeff_b"][None, :], E.deg)[0]
            rec = g[f"{group_name}/bases_seq_0_16"]
            cw = rec.shape[1] // 3
            self.base = []
            for row in rec:
                X, Y, Z = (from_words(F, row[None, j * cw:(j + 1) * cw], E.deg)[0] for j in range(3))
                zi = E.inv(Z)
                if group_name.startswith("bw6_761"):   # homogeneous projective records
                    self.base.append((E.mul(X, zi), E.mul(Y, zi)))
                else:                                  # Jacobian records
                    zi2 = E.mul(zi, zi)
                    self.base.append((E.mul(X, zi2), E.mul(Y, E.mul(zi2, zi))))
        assert all(self.on_curve(P) for P in self.base) and len(set(self.base)) == 16

    def on_curve(self, P):
        E = self.E
        x, y = P
        rhs = E.add(E.add(E.mul(E.mul(x, x), x), E.mul(self.a, x)), self.b)
        return E.mul(y, y) == rhs

    def neg(self, P):
        return INF if P is INF else (P[0], self.E.neg(P[1]))

    def add(self, P, Q):
        E = self.E
        if P is INF:
            return Q
        if Q is INF:
            return P
        if P[0] == Q[0]:
            if E.add(P[1], Q[1]) == E.zero():
                return INF
            xx = E.mul(P[0], P[0])
            lam = E.mul(E.add(E.add(E.add(xx, xx), xx), self.a), E.inv(E.add(P[1], P[1])))
        else:
            lam = E.mul(E.sub(Q[1], P[1]), E.inv(E.sub(Q[0], P[0])))
        x = E.sub(E.sub(E.mul(lam, lam), P[0]), Q[0])
        return (x, E.sub(E.mul(lam, E.sub(P[0], x)), P[1]))

    def xyzz(self, P, z):
        """(X, Y, ZZ, ZZZ) of P scaled by z; infinity: ZZ = 0"""
        E = self.E
        if P is INF:
            return (z, z, E.zero(), E.zero())
        zz = E.mul(z, z)
        zzz = E.mul(zz, z)
        return (E.mul(P[0], zz), E.mul(P[1], zzz), zz, zzz)

    def of_xyzz(self, rec):
        """affine point of an (X, Y, ZZ, ZZZ) record in any representatives; checks ZZ^3 == ZZZ^2"""
        E, p = self.E, self.E.F.p
        X, Y, ZZ, ZZZ = (tuple(c % p for c in e) for e in rec)
        if ZZ == E.zero():
            return INF
        assert E.mul(E.mul(ZZ, ZZ), ZZ) == E.mul(ZZZ, ZZZ), "ZZ^3 != ZZZ^2"
        return (E.mul(X, E.inv(ZZ)), E.mul(Y, E.inv(ZZZ)))

    def of_jac(self, rec):
        E = self.E
        X, Y, Z = rec[:3]
        if Z == E.zero():
            return INF
        zi = E.inv(Z)
        zi2 = E.mul(zi, zi)
        return (E.mul(X, zi2), E.mul(Y, E.mul(zi2, zi)))


@functools.lru_cache(maxsize=None)
def curve(group_name):
    return CurveModel(group_name)


@functools.lru_cache(maxsize=None)
def point_cases(group_name, op):
    """-> (acc records, second operands or None, expected affine points).  acc: tuples of four elements; madd_lz: each
    component as v or v + p, infinity marked by ZZ = 0 and by ZZ = p, so that P = U2 - X1 of an equal or opposite point
    comes out as 0 and as p whichever representative the device's U2 takes."""
    C = curve(group_name)
    E, p = C.E, C.E.F.p
    rng = random.Random(f"{group_name}/{op}")
    rz = lambda: tuple(rng.randrange(1, p) for _ in range(E.deg))
    A = [C.add(C.base[j % 16], C.add(C.base[(j // 16 + j + 1) % 16], C.base[(3 * j + 5) % 16])) for j in range(64)]
    assert all(P is not INF and C.on_curve(P) for P in A)
    aff_inf = (E.zero(), E.zero())
    acc, sec, want = [], [], []

    def reps(rec):
        if op != "madd_lz":
            return [rec]
        out = [rec, tuple(tuple(c + p for c in e) for e in rec)]   # all canonical, all shifted
        out += [tuple(tuple(c + p * rng.randrange(2) for c in e) for e in rec) for _ in range(2)]
        return out

    for j, P in enumerate(A):
        Q = A[(j + 7) % 64]
        if op in ("madd_lz", "madd"):
            for other in (Q, P, C.neg(P)):
                for r in reps(C.xyzz(P, rz())):
                    acc.append(r), sec.append(other), want.append(C.add(P, other))
        elif op == "add":
            for other in (Q, P, C.neg(P)):
                acc.append(C.xyzz(P, rz())), sec.append(C.xyzz(other, rz())), want.append(C.add(P, other))
        elif op in ("dbl", "to_jac"):
            acc.append(C.xyzz(P, rz())), sec.append(None), want.append(C.add(P, P) if op == "dbl" else P)
        else:   # dbl_affine
            acc.append(C.xyzz(INF, rz())), sec.append(P), want.append(C.add(P, P))
    P = A[0]
    if op in ("madd_lz", "madd"):
        for r in reps(C.xyzz(INF, rz())):                    # infinity + P; madd_lz: ZZ = 0 and ZZ = p
            acc.append(r), sec.append(P), want.append(P)
        for r in reps(C.xyzz(P, rz())):                      # P + infinity
            acc.append(r), sec.append(aff_inf), want.append(P)
        acc.append(C.xyzz(INF, rz())), sec.append(aff_inf), want.append(INF)
    elif op == "add":
        inf = lambda: C.xyzz(INF, rz())
        for a_, b_, w in ((inf(), C.xyzz(P, rz()), P), (C.xyzz(P, rz()), inf(), P), (inf(), inf(), INF)):
            acc.append(a_), sec.append(b_), want.append(w)
    elif op in ("dbl", "to_jac"):
        acc.append(C.xyzz(INF, rz())), sec.append(None), want.append(INF)
    return acc, (None if sec[0] is None else sec), want
