"""Interval walk of the loose 28-bit-limb Horner chain (libff_amd/csrc/wide28.cuh: mul28, carry28, the lifted-p
subtractions, jac_dbl_28, jac_add_28, to28 / from28), in the manner of tests/test_rr_bounds.py.

The chain never normalises between its first and its last conversion; what makes that exact is a set of bounds the
header states and pins with static_asserts.  This test re-derives them mechanically for the three moduli of the lazy
chain: it carries, per element, the largest limb below the top one, the largest top limb and the largest value (an exact
fraction of p) through the operation sequences of the doubling and of the addition -- mirrored by hand, same order of
operations, same carry steps: a change there must be repeated here -- over arbitrary interleavings: the domain of a
running point is the hull of a converted point, the doubling of anything in the domain and the sum of any two elements of
the domain (addition after addition, doubling after addition, the doubling the addition falls back to), iterated until
it stops growing.  Asserted on the way: every 64-bit column of mul28 below 2^64, every shifted column and every limb
below 2^32, every product operand within the limb bound mul28 documents (2^29.7), every lifted multiple of p above its
subtrahend limb by limb, every result an exact test normalises below 2 p.  CPU only, no device code involved."""
import math
from fractions import Fraction

import pytest

MODULI = {
    "alt_bn128": 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
    "bls12_377": 0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001,
    "bls12_381": 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
}
MASK = (1 << 28) - 1
OPERAND_LIMB = int(2 ** 29.7)   # "operand limbs < 2^29.7" (mul28)
HEAD = 10


class El:
    """worst case of one element: largest limb 0..L-2, largest top limb, largest value in units of p"""

    def __init__(self, limb, top, val):
        self.limb, self.top, self.val = int(limb), int(top), Fraction(val)

    def __repr__(self):
        return f"El(limb 2^{self.limb.bit_length()}, top {self.top}, value {float(self.val):.3f} p)"


def hull(a, b):
    return El(max(a.limb, b.limb), max(a.top, b.top), max(a.val, b.val))


def same(a, b):
    return (a.limb, a.top, a.val) == (b.limb, b.top, b.val)


class Walk:
    def __init__(self, p):
        self.p = p
        bits = p.bit_length()
        self.L = (bits + HEAD + 27) // 28
        self.J = (bits - 1) // 28
        assert self.J == self.L - 1 and self.L < 16
        self.R = 1 << (28 * self.L)
        assert self.R >= (p << HEAD)
        self.plimbs = self.limbs(p)
        self.stats = {"column": 0, "shifted": 0, "operand": 0, "limb": 0}

    def limbs(self, x):
        return [(x >> (28 * j)) & MASK if j < self.L - 1 else x >> (28 * j) for j in range(self.L)]

    def lifted(self, log2k, lift=30):
        """W28::lifted"""
        t = self.limbs(self.p << log2k)
        for j in range(self.J + 1):
            t[j] += ((1 << lift) if j < self.J else 0) - ((1 << (lift - 28)) if j > 0 else 0)
        assert sum(v << (28 * j) for j, v in enumerate(t)) == self.p << log2k
        return t

    def top_of(self, e):
        """the top limb cannot exceed the value's own (lower limbs are non-negative)"""
        return min(e.top, int(e.val * self.p) >> (28 * self.J))

    def limb_ok(self, x):
        assert x < 1 << 32, x
        self.stats["limb"] = max(self.stats["limb"], x)
        return x

    def add(self, *es):
        return El(self.limb_ok(sum(e.limb for e in es)), self.limb_ok(sum(self.top_of(e) for e in es)), sum(e.val for e in es))

    def carry(self, e):
        """carry28: every lane below the top hands its bits >= 28 up"""
        c = e.limb >> 28
        return El(self.limb_ok(MASK + c), self.limb_ok(self.top_of(e) + c), e.val)

    def sub(self, a, b, log2k):
        """carry28(a + K p lifted - b)"""
        kp = self.lifted(log2k)
        for j in range(self.J):
            assert b.limb <= kp[j], ("lifted limb below the subtrahend's", j, b)
        assert self.top_of(b) <= kp[self.J], ("top limb of K p below the subtrahend's", log2k, b)
        raw = El(self.limb_ok(a.limb + max(kp[:self.J])), self.limb_ok(self.top_of(a) + kp[self.J]), a.val + (1 << log2k))
        return self.carry(raw)

    def mul(self, a, b):
        """mul28: L steps of A = a b_i + t, B = m p + A, t = (B >> 28) + (B & MASK of the lane above), then carry28"""
        for e in (a, b):
            m = max(e.limb, self.top_of(e))
            assert m < OPERAND_LIMB, ("operand limb", e)
            self.stats["operand"] = max(self.stats["operand"], m)
        amax, bmax = max(a.limb, self.top_of(a)), max(b.limb, self.top_of(b))
        t = 0
        for _ in range(self.L):
            A = amax * bmax + t
            B = MASK * max(self.plimbs) + A
            assert B < 1 << 64
            self.stats["column"] = max(self.stats["column"], B)
            t = (B >> 28) + MASK
            assert t < 1 << 32
            self.stats["shifted"] = max(self.stats["shifted"], t)
        # rounded up to a multiple of 2^-16 p: the walk then moves on a finite grid and reaches its fixed point exactly
        val = Fraction(math.ceil(a.val * b.val * self.p * (1 << 16) / self.R), 1 << 16) + 1
        out = El(0, 0, val)
        out.top = int(val * self.p) >> (28 * self.J)
        out.limb = self.limb_ok(MASK + (t >> 28))
        assert out.limb <= (1 << 28) + (1 << 5)
        return out

    def exact(self, e):
        """exact28 / from28: the result of a product, below 2 p, limbs below 2^28 + 2^5, top limb below 2^28"""
        assert e.val <= 2 and e.limb <= (1 << 28) + (1 << 5) and self.top_of(e) + 1 < 1 << 28, e

    # ---- conversions
    def to28(self):
        w = El(MASK, MASK, 1)                                   # regrouped canonical words, value < p
        cin = El(MASK, MASK, 1)
        return self.mul(w, cin)

    def from28(self, e):
        assert e.val * self.p < self.R >> 2
        r = self.mul(e, El(MASK, MASK, 1))
        self.exact(r)

    # ---- jac_dbl_28
    def dbl(self, X, Y, Z):
        XX, B, YZ = self.mul(X, X), self.mul(Y, Y), self.mul(Y, Z)
        B2, E3 = self.add(B, B), self.add(XX, XX, XX)
        C4, XB2, F = self.mul(B2, B2), self.mul(X, B2), self.mul(E3, E3)
        D = self.add(XB2, XB2)
        X3 = self.sub(F, self.add(D, D), 4)
        t = self.mul(E3, self.sub(D, X3, 5))
        Y3 = self.sub(t, self.add(C4, C4), 4)
        Z3 = self.add(YZ, YZ)
        return X3, Y3, Z3

    # ---- jac_add_28 (both operands from the same domain); returns the outputs of its two computing paths
    def addp(self, P1, P2):
        (X1, Y1, Z1), (X2, Y2, Z2) = P1, P2
        z1z1, z2z2, z1z2 = self.mul(Z1, Z1), self.mul(Z2, Z2), self.mul(Z1, Z2)
        self.exact(z1z1)
        self.exact(z2z2)
        u1, u2, t1, t2 = self.mul(X1, z2z2), self.mul(X2, z1z1), self.mul(Z2, z2z2), self.mul(Z1, z1z1)
        h = self.sub(u2, u1, 2)
        h2 = self.add(h, h)
        s1, s2, ii, zh = self.mul(Y1, t1), self.mul(Y2, t2), self.mul(h2, h2), self.mul(z1z2, h)
        self.exact(ii)
        d = self.sub(s2, s1, 2)
        rr = self.add(d, d)
        unit = El(MASK, MASK, 1)
        self.exact(self.mul(rr, unit))                          # the r == 0 test
        fall = self.dbl(X1, Y1, Z1)                             # the same point: jac_dbl_28 ...
        self.exact(self.mul(fall[2], unit))                     # ... and the exact test of its Z
        J, V, R2 = self.mul(h, ii), self.mul(u1, ii), self.mul(rr, rr)
        X3 = self.sub(R2, self.add(J, V, V), 4)
        t = self.mul(rr, self.sub(V, X3, 5))
        sj = self.mul(s1, J)
        Y3 = self.sub(t, self.add(sj, sj), 4)
        Z3 = self.add(zh, zh)
        return (X3, Y3, Z3), fall


@pytest.mark.parametrize("name", list(MODULI))
def test_lazy_chain_bounds_close(name):
    w = Walk(MODULI[name])
    # 2^(28 L) >= 2^10 p: products of operands up to 36 p stay below 2.3 p, of the addition's operands below 1.4 p
    c = w.to28()
    dom = (c, c, c)
    for it in range(40):
        d = w.dbl(*dom)
        a, f = w.addp(dom, dom)
        new = tuple(hull(hull(dom[i], d[i]), hull(a[i], f[i])) for i in range(3))
        if all(same(new[i], dom[i]) for i in range(3)):
            break
        dom = new
    else:
        pytest.fail(f"the bounds keep growing: {dom}")
    X, Y, Z = dom
    print(f"{name}: L = {w.L}, fixed point after {it} rounds: X {X}, Y {Y}, Z {Z}; largest column 2^{w.stats['column'].bit_length()}, "
          f"shifted column {w.stats['shifted']}, operand limb {w.stats['operand']}, limb {w.stats['limb']}")
    # the domain wide28.cuh states for a running point: X, Y < 19 p, Z < 4 p, limbs < 2^29.1
    assert X.val < 19 and Y.val < 19 and Z.val < 4
    assert max(X.limb, Y.limb, Z.limb) < 2 ** 29.1
    # the addition alone (what its header line says): X3 < 17.1 p, Y3 < 17.33 p, Z3 < 2.02 p from the full domain
    a, _ = w.addp(dom, dom)
    assert a[0].val < Fraction(171, 10) and a[1].val < Fraction(1733, 100) and a[2].val < Fraction(202, 100)
    # the last conversion: any coordinate of the domain
    for e in dom:
        w.from28(e)
    assert w.stats["column"] < 1 << 64 and w.stats["shifted"] < 1 << 32 and w.stats["limb"] < 1 << 32


@pytest.mark.parametrize("name", list(MODULI))
def test_lifted_constants_cover_their_subtrahends(name):
    """4 p / 16 p / 32 p lifted by 2^30: limb by limb above any subtrahend below 2 p / 8 p / 18 p with limbs below 2^30 - 4"""
    w = Walk(MODULI[name])
    ptop = (w.p >> (28 * w.J)) + 1
    for log2k, s in ((2, 2), (4, 8), (5, 18)):
        kp = w.lifted(log2k)
        assert all(kp[j] >= (1 << 30) - 4 for j in range(w.J))
        assert kp[w.J] >= ptop * s
        assert max(kp) + (1 << 28) + (1 << 5) < 1 << 32


def test_walk_rejects_what_the_code_must_not_do():
    """the checker is not vacuous: an uncovered subtrahend and an oversized operand are refused"""
    w = Walk(MODULI["alt_bn128"])
    c = w.to28()
    big = El(MASK + 8, 0, 19)
    big.top = int(big.val * w.p) >> (28 * w.J)
    with pytest.raises(AssertionError):
        w.sub(c, big, 2)            # 4 p cannot serve a subtrahend of 19 p
    wide = El(4 * MASK, 1, 2)
    with pytest.raises(AssertionError):
        w.mul(wide, wide)           # 2^30 limbs are no product operands
