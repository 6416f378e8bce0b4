"""Cases and expectations of the fixed-base batch_exp tests (tests/test_gpu_batch_exp.py), device-free: the CPU tests
(tests/test_fixed_base_cases_cpu.py) prove them against the oracle's batch_exp and the MNT model's windowed loop.

An expectation is the closed form of libff's batch_exp / batch_exp_with_coeff (multiexp.tcc:874-947): for scalars below
2^scalar_size the window table only regroups the bits of v, so out[i] = k_i g with k_i = v_i, or coeff v_i mod r with a
coefficient -- one scalar multiplication per element, by the oracle (oracle/port.py) for the eight pairing-curve groups
and by tests/mnt_model.py for the three MNT groups.  Results are compared as affine points, every element."""
import random

import numpy as np

import ffi_wire
import mnt_model as mm
from common import GROUPS, golden, to_int

ALL_GROUPS = [g[0] for g in GROUPS] + ["mnt4_g1", "mnt4_g2", "mnt6_g1"]
WORKGROUP_NS = (1, 255, 256, 257, 513)   # one lane per scalar, 256 lanes per workgroup


def _limbs(k, n):
    return [(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


class OracleGroup:
    """one of the eight groups of oracle/port.py"""

    def __init__(self, port, name):
        self.port, self.name = port, name
        _, self.curve, self.group = next(g for g in GROUPS if g[0] == name)
        s = port.sizes(self.curve, self.group)
        self.bits, self.limbs = s["fr_bits"], s["fr_bytes"] // 8
        self.r = to_int(golden()[f"{name}/fr_modulus"])
        assert self.r.bit_length() == self.bits
        self.one, self.zero = port.group_consts(self.curve, self.group)

    def scalars(self, ks, plain):
        a = np.array([_limbs(k, self.limbs) for k in ks], dtype=np.uint64).reshape(len(ks), self.limbs)
        if plain:
            return a
        assert all(k < self.r for k in ks), "a Montgomery record holds a value below r"
        return self.port.fr_from_bigint(self.curve, a) if len(ks) else a

    def mul(self, k, g, in_subgroup=True):
        """k g by the oracle's scalar multiplication (curve_utils.tcc:14-32); k is reduced mod r only where g has order r"""
        if in_subgroup:
            k %= self.r
        assert k < self.r
        return self.port.scalar_mul(self.curve, self.group, g, self.scalars([k], False)[0])

    def neg(self, g):
        return self.port.group_op(self.curve, self.group, 3, g)

    def multiple_not_normalised(self, k):
        """3 (k G) as the addition leaves it, Z != 1 (on bw6_761 the projective form)"""
        p = self.mul(k, self.one)
        p = self.port.group_op(self.curve, self.group, 4, p)
        q = self.port.group_op(self.curve, self.group, 0, self.port.group_op(self.curve, self.group, 2, p), p)
        assert (q != self.port.group_op(self.curve, self.group, 4, q)).any()
        return q

    def keys(self, rows):
        """the affine form of every record, comparable"""
        return [self.port.group_op(self.curve, self.group, 4, x).tobytes() for x in rows]

    def outside_subgroup(self):
        cp, flags = golden()[f"{self.name}/curve_points"], golden()[f"{self.name}/curve_points_flags"]
        for p, f in zip(cp, flags):
            if (int(f) & 3) == 1:
                return p
        return None

    def order_two(self):
        x_plain = {"bls12_377_g1": -1, "bw6_761_g1": 1}.get(self.name)
        if x_plain is None:
            return None
        q = to_int(golden()[f"{self.name}/fq_modulus"])
        nq = len(golden()[f"{self.name}/fq_modulus"])
        r_mont = (1 << (64 * nq)) % q
        t = np.array(_limbs(x_plain * r_mont % q, nq) + _limbs(0, nq) + _limbs(r_mont, nq), dtype=np.uint64)
        assert self.port.group_op(self.curve, self.group, 6, self.port.group_op(self.curve, self.group, 2, t), self.zero) != 0
        return t


class MntGroup:
    """one of the three groups of tests/mnt_model.py; records are its libff records, keys its affine points"""

    def __init__(self, name):
        self.name = name
        self.model, self.curve, self.group = ffi_wire.MNT_GROUPS[name]
        self.r, self.bits, self.limbs = self.model.r, self.model.r.bit_length(), mm.WORDS
        self.one, self.zero = self.model.records([self.model.one])[0], self.model.records([mm.INF])[0]
        self._doublings = {}

    def scalars(self, ks, plain):
        if plain:
            return self.model.scalars_plain(ks)
        assert all(k < self.r for k in ks), "a Montgomery record holds a value below r"
        return self.model.scalars_mont(ks)

    def mul(self, k, g, in_subgroup=True):
        """k g, double and add over the doublings of g (kept: every element of a batch shares them)"""
        if in_subgroup:
            k %= self.r
        P = self.model.point(g)
        dbl = self._doublings.setdefault(P, [P])
        R, j = mm.INF, 0
        while k:
            if len(dbl) <= j:
                dbl.append(self.model.add(dbl[-1], dbl[-1]))
            if k & 1:
                R = self.model.add(R, dbl[j])
            k >>= 1
            j += 1
        return self.model.records([R])[0]

    def neg(self, g):
        return self.model.records([self.model.neg(self.model.point(g))])[0]

    def multiple_not_normalised(self, k):
        return self.model.records([self.model.mul(3 * k, self.model.one)], [0x1234567])[0]

    def keys(self, rows):
        return [self.model.point(x) for x in rows]

    def outside_subgroup(self):
        f = ffi_wire.fixtures()
        for b, ok in zip(f[f"{self.name}/curve_points"], f[f"{self.name}/curve_points_ok"]):
            if not ok:
                P = ffi_wire.decode_point(self.model, b)
                assert self.model.on_curve(P) and not ffi_wire.in_subgroup(self.model, P)
                return self.model.records([P])[0]
        return None

    def order_two(self):
        return None


def group_of(port, name):
    return MntGroup(name) if name.startswith("mnt") else OracleGroup(port, name)


# ---- table shapes
def table_shapes(bits, limbs):
    """(scalar_size, window) of the table-shape cases: 2 b entries ragged against the 32 one lane normalises; window 2;
    a full last row of four; a last row of two entries; one row of two entries; the largest scalar_size the entry
    accepts; the shape bench.py times"""
    return [(bits, 1), (bits, 2), (64, 16), (65, 16), (1, 1), (64 * limbs, 13), (bits, 17)]


def row_lengths(scalar_size, window):
    """entries per row of get_window_table (multiexp.tcc:809-846): 2^window, the last row 2^(bits left)"""
    outerc = (scalar_size + window - 1) // window
    return [1 << window] * (outerc - 1) + [1 << (scalar_size - (outerc - 1) * window)]


def scalar_values(scalar_size, window, r, seed, n=None, below_r=False):
    """n integers below 2^scalar_size: the edge values of one table shape, filled up with seeded random ones.
    0 and 1; every power 2^k at a window's first or last bit (one nonzero digit, the accumulator infinite up to it);
    2^scalar_size - 1 (the last entry of every row); digits alternating between zero and nonzero, both phases; the lowest
    two windows zero; r - 1.  below_r: only values a Montgomery record (or a product with a coefficient) can hold.
    Where n is too small for all the single powers they are thinned evenly, the lowest and the highest kept."""
    rng = random.Random(seed)
    top = 1 << scalar_size
    outerc = (scalar_size + window - 1) // window
    powers = sorted({k for j in range(outerc) for k in (j * window, j * window + window - 1) if k < scalar_size})
    powers = [1 << k for k in powers if not (below_r and 1 << k >= r)]
    vals = [0, 1, top - 1]
    for phase in (0, 1):
        v = 0
        for j in range(outerc):
            if j % 2 == phase:
                v |= rng.randrange(1, 1 << window) << (j * window)
        v %= top
        while below_r and v >= r:   # keep the phase, give up the top two digits
            v >>= 2 * window
        vals.append(v)
    bound = min(top, r)
    if outerc > 2:
        vals.append(rng.randrange(bound >> 1, bound) >> (2 * window) << (2 * window))
    if r < top:
        vals.append(r - 1)
    vals = [v for v in dict.fromkeys(vals) if v < top and not (below_r and v >= r)]
    room = None if n is None else n - len(vals) - 4
    if room is not None and len(powers) > room:
        assert room >= 2, (n, len(vals))
        powers = [powers[i * (len(powers) - 1) // (room - 1)] for i in range(room)]
    vals = list(dict.fromkeys(vals + powers))
    if n is None:   # the edge values and a few random ones, however many that makes
        n = len(vals) + 8
    assert len(vals) <= n, (len(vals), n)
    while len(vals) < n:
        vals.append(rng.randrange(bound))
    return vals


def digits(v, scalar_size, window):
    outerc = (scalar_size + window - 1) // window
    return [(v >> (j * window)) & ((1 << window) - 1) for j in range(outerc)]


def closed_form(grp, g, ks, coeff=None, in_subgroup=True):
    """records of out[i] = k_i g, k_i = v_i or coeff v_i mod r: one scalar multiplication per element"""
    if coeff is not None:
        assert all(k < grp.r for k in ks) and coeff < grp.r
        ks = [coeff * k % grp.r for k in ks]
    return [grp.mul(k, g, in_subgroup) for k in ks]


def order_two_rule(grp, t, ks, coeff=None):
    """for a point t of order two: t where the multiplier is odd, zero where it is even"""
    if coeff is not None:
        ks = [coeff * k % grp.r for k in ks]
    return [t if k & 1 else grp.zero for k in ks]
