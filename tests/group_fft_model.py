"""Integer model of the discrete Fourier transform of a point vector, out[j] = sum_i w^(i j) P_i, for the tests of
Engine.group_fft.  Every input point is a known multiple a_i of the generator G, so output j is e_j G with
e_j = sum_i w^(i j) a_i mod r: the expected records are scalar multiples of G -- oracle.port's scalar_mul for the eight
pairing-curve groups, tests/mnt_model.py for the three MNT groups -- as special-form records.  Nothing here knows the
order of the stages, the index pattern of a butterfly or the window width of the ladder."""
import random

import numpy as np

import mnt_model as mm
from common import GROUPS, golden, to_int

ALL_NAMES = [name for name, _, _ in GROUPS] + ["mnt4_g1", "mnt4_g2", "mnt6_g1"]
CURVE_NAMES = {0: "alt_bn128", 1: "bls12_377", 2: "bw6_761", 3: "bls12_381", 4: "mnt4", 5: "mnt6"}


def _words(v, n):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(n)], dtype=np.uint64)


def dft_logs(logs, w, r):
    """e_j = sum_i w^(i j) a_i mod r, by the definition (n^2 products)"""
    n = len(logs)
    pw = [pow(w, i, r) for i in range(n)]   # w has order n
    return [sum(pw[i * j % n] * a for i, a in enumerate(logs)) % r for j in range(n)]


class PairingGroup:
    """records and expected values through the plain-C restatement"""

    def __init__(self, port, name, curve, group):
        self.port, self.name, self.curve, self.group = port, name, curve, group
        s = port.sizes(curve, group)
        self.fl, self.gl = s["fr_bytes"] // 8, s["g_bytes"] // 8
        self.cl = self.gl // 3
        self.r = to_int(golden()[f"{CURVE_NAMES[curve]}_g1/fr_modulus"])
        self.one, self.zero = port.group_consts(curve, group)
        self.projective = curve == 2   # bw6_761 records are homogeneous projective
        self._mul = {}

    def records(self, logs):
        """special-form records of a G for every a of logs"""
        out = np.zeros((len(logs), self.gl), dtype=np.uint64)
        for i, a in enumerate(logs):
            a %= self.r
            if a not in self._mul:
                p = self.port.scalar_mul(self.curve, self.group, self.one, self.mont([a])[0])
                self._mul[a] = self.port.group_op(self.curve, self.group, 4, p)
            out[i] = self._mul[a]
        return out

    def scale(self, recs, seed):
        """the same points with a random Z each (normal base form)"""
        rng = random.Random(seed)
        cl, out = self.cl, recs.copy()
        mul = lambda a, b: self.port.fq_op(self.curve, self.group, 0, a, b)
        pool = self.records([rng.randrange(1, self.r) for _ in range(4)])
        for i, rec in enumerate(recs):
            if not rec[2 * cl:].any():
                continue
            z = pool[rng.randrange(4)][:cl] if i % 3 else pool[rng.randrange(4)][cl:2 * cl]   # some nonzero field element
            z2 = mul(z, z)
            if self.projective:
                out[i, :cl], out[i, cl:2 * cl] = mul(rec[:cl], z), mul(rec[cl:2 * cl], z)
            else:
                out[i, :cl], out[i, cl:2 * cl] = mul(rec[:cl], z2), mul(rec[cl:2 * cl], mul(z2, z))
            out[i, 2 * cl:] = z
        return out

    def mont(self, ks):
        return self.port.fr_from_bigint(self.curve, np.stack([_words(k % self.r, self.fl) for k in ks]))

    def plain(self, ks):
        return np.stack([_words(k, self.fl) for k in ks])

    def special(self, got):
        return self.port.batch_to_special(self.curve, self.group, got)


class MntGroup:
    """records and expected values through the integer model of the curve: a G from a table of d 16^w G by additions"""

    def __init__(self, name, curve, group, model):
        self.name, self.curve, self.group, self.model = name, curve, group, model
        self.r, self.fl, self.gl = model.r, mm.WORDS, 3 * model.cw
        self._mul, self._table = {0: mm.INF}, None

    def _mul_g(self, e):
        m = self.model
        e %= m.r
        if e not in self._mul:
            if e > m.r // 2:
                self._mul[e] = m.neg(self._mul_g(m.r - e))
            else:
                if self._table is None:
                    self._table, base = [], m.one
                    for _ in range((m.r.bit_length() + 3) // 4):
                        row, P = [mm.INF], mm.INF
                        for _ in range(15):
                            P = m.add(P, base)
                            row.append(P)
                        self._table.append(row)
                        base = m.add(P, base)
                acc, w, v = mm.INF, 0, e
                while v:
                    acc = m.add(acc, self._table[w][v & 15])
                    v >>= 4
                    w += 1
                self._mul[e] = acc
        return self._mul[e]

    def records(self, logs, zs=None):
        return self.model.records([self._mul_g(a) for a in logs], zs)

    def scale(self, recs, seed):
        rng = random.Random(seed)
        return self.model.records([self.model.point(r) for r in recs], [rng.randrange(1, self.model.p) for _ in recs])

    def mont(self, ks):
        return self.model.scalars_mont(ks)

    def plain(self, ks):
        return np.stack([_words(k, self.fl) for k in ks])

    def special(self, got):
        return self.model.records([self.model.point(r) for r in got])


_groups = {}


def group_of(port, name):
    if name not in _groups:
        pairing = {g[0]: g for g in GROUPS}
        if name in pairing:
            _groups[name] = PairingGroup(port, *pairing[name])
        else:
            curve, group, model = {"mnt4_g1": (4, 1, mm.MNT4), "mnt4_g2": (4, 2, mm.MNT4_G2), "mnt6_g1": (5, 1, mm.MNT6)}[name]
            _groups[name] = MntGroup(name, curve, group, model)
    return _groups[name]


_cases = {}


def case(port, name, logs, w):
    """(group, the inputs a_i G as special-form records, the expected outputs as special-form records) of the transform of
    the multipliers `logs` with the root `w`: computed once, shared by the tests and never changed"""
    key = (name, tuple(logs), w)
    if key not in _cases:
        g = group_of(port, name)
        pts, want = g.records(logs), g.records(dft_logs(logs, w, g.r))
        pts.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (g, pts, want)
    return _cases[key]
