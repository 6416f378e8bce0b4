"""Pure-integer model of MNT4-298 G1 / G2 and MNT6-298 G1 (y^2 = x^3 + a x + b, a != 0; MNT4 G2 over
Fq2 = Fq[u]/(u^2 - 17) with a' = 34, b' = (0, 17 b)) and of the engine's record layouts
for them: Montgomery coordinates with R = 2^320 (libff's bigint<5>), libff records (X : Y : Z) homogeneous
projective, scalars of Fr as five 64-bit words.  The curve constants are the generator's (tools/gen_params.py
MNT_CURVES, the values of mnt4_init.cpp / mnt6_init.cpp); every other value is derived here.  It is the closed-form
checker of the MNT tests, which run where the reference is not available."""
import importlib.util
import os
import random

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("amdmsm_gen_params", os.path.join(_ROOT, "tools", "gen_params.py"))
_gp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gp)

WORDS = 5            # 64-bit words per Fq / Fr element
RADIX = 1 << 320     # Montgomery radix
INF = None           # the point at infinity


class Fq:
    """the prime field as plain integers"""
    deg = 1

    def __init__(self, p):
        self.p = p

    def c(self, v):
        return v % self.p

    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def mul(self, a, b):
        return a * b % self.p

    def inv(self, a):
        return pow(a, -1, self.p)

    def zero(self):
        return 0

    def comps(self, a):
        return [a]

    def of_comps(self, cs):
        return cs[0] % self.p


class Fq2(Fq):
    """Fq[u]/(u^2 - nr) as pairs (c0, c1)"""
    deg = 2

    def __init__(self, p, nr):
        self.p, self.nr = p, nr

    def c(self, v):
        return (v % self.p, 0)

    def add(self, a, b):
        return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)

    def sub(self, a, b):
        return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)

    def mul(self, a, b):
        p = self.p
        return ((a[0] * b[0] + self.nr * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def inv(self, a):
        p = self.p
        t = pow((a[0] * a[0] - self.nr * a[1] * a[1]) % p, -1, p)
        return (a[0] * t % p, -a[1] * t % p)

    def zero(self):
        return (0, 0)

    def comps(self, a):
        return list(a)

    def of_comps(self, cs):
        return (cs[0] % self.p, cs[1] % self.p)


class Curve:
    def __init__(self, name, group="g1"):
        c = _gp.MNT_CURVES[name]
        g = c[group]
        self.name, self.id = f"{name}_{group}", c["id"]
        self.p, self.r = c["q"], c["r"]
        if g["deg"] == 1:
            self.F = Fq(self.p)
            self.a, self.b = g["a"], g["b"][0]
            self.one = (g["x"][0], g["y"][0])
        else:   # the twist: a' = a (a small integer of Fq), b' = (0, b * nr)
            self.F = Fq2(self.p, g["nr"])
            self.a = (g["a"], 0)
            self.b = (0, c["g1"]["b"][0] * g["nr"] % self.p)
            self.one = (tuple(g["x"]), tuple(g["y"]))
        self.deg = g["deg"]
        self.cw = WORDS * self.deg   # 64-bit words per coordinate
        assert self.on_curve(self.one)

    # ---- group law, affine, None = infinity
    def on_curve(self, P):
        if P is INF:
            return True
        F = self.F
        x, y = P
        rhs = F.add(F.add(F.mul(F.mul(x, x), x), F.mul(F.c(self.a) if self.deg == 1 else self.a, x)),
                    F.c(self.b) if self.deg == 1 else self.b)
        return F.sub(F.mul(y, y), rhs) == F.zero()

    def neg(self, P):
        return INF if P is INF else (P[0], self.F.sub(self.F.zero(), P[1]))

    def add(self, P, Q):
        F = self.F
        if P is INF:
            return Q
        if Q is INF:
            return P
        if P[0] == Q[0]:
            if F.add(P[1], Q[1]) == F.zero():
                return INF
            xx = F.mul(P[0], P[0])
            num = F.add(F.add(F.add(xx, xx), xx), F.c(self.a) if self.deg == 1 else self.a)
            lam = F.mul(num, F.inv(F.add(P[1], P[1])))
        else:
            lam = F.mul(F.sub(Q[1], P[1]), F.inv(F.sub(Q[0], P[0])))
        x = F.sub(F.sub(F.mul(lam, lam), P[0]), Q[0])
        return (x, F.sub(F.mul(lam, F.sub(P[0], x)), P[1]))

    def dbl(self, P):
        return self.add(P, P)

    def mul(self, k, P):
        k %= self.r
        R = INF
        while k:
            if k & 1:
                R = self.add(R, P)
            P = self.add(P, P)
            k >>= 1
        return R

    def msm(self, bases, scalars):
        acc = INF
        for P, k in zip(bases, scalars):
            acc = self.add(acc, self.mul(k, P))
        return acc

    # ---- layouts
    def fq_mont(self, v):
        return v * RADIX % self.p

    def fq_from_mont(self, v):
        return v * pow(RADIX, -1, self.p) % self.p

    def _coord_words(self, v):
        return np.concatenate([words(self.fq_mont(c)) for c in self.F.comps(v)])

    def _coord_of_words(self, ws):
        return self.F.of_comps([self.fq_from_mont(to_int(ws[i * WORDS:(i + 1) * WORDS])) for i in range(self.deg)])

    def record(self, P, z=1):
        """libff record (X : Y : Z) in Montgomery form; z != 1 scales a finite point (normal base form)"""
        F = self.F
        if P is INF:
            return [F.zero(), F.c(1), F.zero()]
        zz = F.c(z)
        return [F.mul(P[0], zz), F.mul(P[1], zz), zz]

    def records(self, pts, zs=None):
        out = np.zeros((len(pts), 3 * self.cw), dtype=np.uint64)
        for i, P in enumerate(pts):
            for j, v in enumerate(self.record(P, 1 if zs is None else zs[i])):
                out[i, j * self.cw:(j + 1) * self.cw] = self._coord_words(v)
        return out

    def point(self, row):
        """libff record (homogeneous projective, Montgomery) -> affine point"""
        F = self.F
        X, Y, Z = (self._coord_of_words(row[j * self.cw:(j + 1) * self.cw]) for j in range(3))
        if Z == F.zero():
            return INF
        zi = F.inv(Z)
        P = (F.mul(X, zi), F.mul(Y, zi))
        assert self.on_curve(P), "result off the curve"
        return P

    def disk_write(self, pts):
        """libff's on-disk records of the points, group_write<encoding_binary, form_montgomery, compression_off>
        (curve_serialization.tcc:78-101): affine X then Y, every Fq component (c0 before c1) the Montgomery residue as
        8 * WORDS big-endian bytes (field_serialization.tcc:125-208); zero is (0, one)"""
        F = self.F
        out = bytearray()
        for P in pts:
            for v in ((F.zero(), F.c(1)) if P is INF else P):
                for c in F.comps(v):
                    out += self.fq_mont(c).to_bytes(8 * WORDS, "big")
        return bytes(out)

    def scalars_plain(self, ks):
        out = np.zeros((len(ks), WORDS), dtype=np.uint64)
        for i, k in enumerate(ks):
            out[i] = words(k)
        return out

    def scalars_mont(self, ks):
        rr = RADIX % self.r
        out = np.zeros((len(ks), WORDS), dtype=np.uint64)
        for i, k in enumerate(ks):
            out[i] = words(k % self.r * rr % self.r)
        return out

    def random_points(self, n, seed):
        rng = random.Random(seed)
        return [self.mul(rng.randrange(1, self.r), self.one) for _ in range(n)]


def words(v, n=WORDS):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(n)], dtype=np.uint64)


def to_int(ws):
    return sum(int(w) << (64 * i) for i, w in enumerate(ws))


MNT4 = Curve("mnt4")
MNT4_G2 = Curve("mnt4", "g2")
MNT6 = Curve("mnt6")
CURVES = {"mnt4": MNT4, "mnt4_g2": MNT4_G2, "mnt6": MNT6}
