"""Integer model of the sparse matrix times vector that Engine.fr_matrix_apply computes,

    out[i] = sum over offsets[i] <= k < offsets[i + 1] of coeffs[k] * x[cols[k]]   (mod r),   i < n_rows
    out[i] = 0,                                                                               n_rows <= i < n_out,

for the tests of the Fr matrix entries: the CSR loop, the dense double loop it is checked against in the CPU suite, the
class counts the plan entry reports, and the two record forms (fr_fft_model.Field).  Python integers only.  Nothing
here knows how the library stores a matrix or in what order it adds."""
import random

import numpy as np

from fr_fft_model import CURVES, field  # noqa: F401


class Csr:
    """rows: a list of rows, each a list of (column, coefficient) with integer coefficients in [0, r)"""

    def __init__(self, rows, n_cols):
        self.rows, self.n_cols, self.n_rows = rows, n_cols, len(rows)
        self.offsets = [0]
        for row in rows:
            self.offsets.append(self.offsets[-1] + len(row))
        self.cols = [c for row in rows for c, _ in row]
        self.coeffs = [v for row in rows for _, v in row]
        self.nnz = len(self.cols)

    def arrays(self, f, plain):
        """(offsets, cols, coefficient records) as Engine.fr_matrix_load takes them"""
        recs = f.records(self.coeffs, plain) if self.nnz else np.zeros((0, f.limbs), dtype=np.uint64)
        return np.array(self.offsets, dtype=np.uint64), np.array(self.cols, dtype=np.uint32), recs


def apply(m, x, r, n_out=None):
    """the definition over the CSR arrays"""
    n_out = m.n_rows if n_out is None else n_out
    assert n_out >= m.n_rows and len(x) >= m.n_cols
    out = []
    for i in range(m.n_rows):
        acc = 0
        for k in range(m.offsets[i], m.offsets[i + 1]):
            acc += m.coeffs[k] * x[m.cols[k]]
        out.append(acc % r)
    return out + [0] * (n_out - m.n_rows)


def dense(m, r):
    """the matrix as n_rows x n_cols integers, repeated columns added up"""
    d = [[0] * m.n_cols for _ in range(m.n_rows)]
    for i, row in enumerate(m.rows):
        for c, v in row:
            d[i][c] = (d[i][c] + v) % r
    return d


def apply_dense(m, x, r, n_out=None):
    """the same values by the dense double loop"""
    n_out = m.n_rows if n_out is None else n_out
    d = dense(m, r)
    return [sum(d[i][j] * x[j] for j in range(m.n_cols)) % r for i in range(m.n_rows)] + [0] * (n_out - m.n_rows)


def class_counts(m, r):
    """entries by coefficient class, as amdmsm_plan_fr_matrix reports them"""
    c = {"general": 0, "plus_one": 0, "minus_one": 0, "zero": 0}
    for v in m.coeffs:
        c["zero" if v == 0 else "plus_one" if v == 1 else "minus_one" if v == r - 1 else "general"] += 1
    return c


def row_lengths(m):
    """the number of non-zero entries of every row: what the library classes rows by"""
    return [sum(1 for _, v in row if v) for row in m.rows]


def pick_coeff(rng, r):
    """0, 1, r - 1, 2, r - 2, a power of two or a random value"""
    k = rng.randrange(10)
    if k < 5:
        return (0, 1, r - 1, 2, r - 2)[k]
    if k < 7:
        return pow(2, rng.randrange(2, r.bit_length() + 40), r)
    return rng.randrange(r)


def pick_x(rng, r):
    k = rng.randrange(8)
    return (0, 1, r - 1)[k] if k < 3 else rng.randrange(r)


def random_matrix(r, lengths, n_cols, seed, nonzero=True):
    """a row of `lengths[i]` entries each; nonzero: no zero coefficients, so the lengths are also the kept lengths"""
    rng = random.Random(seed)
    rows = []
    for n in lengths:
        row = []
        for _ in range(n):
            v = pick_coeff(rng, r)
            while nonzero and v == 0:
                v = pick_coeff(rng, r)
            row.append((rng.randrange(n_cols), v))
        rows.append(row)
    return Csr(rows, n_cols)


def random_x(r, n, seed):
    rng = random.Random(seed)
    return [pick_x(rng, r) for _ in range(n)]


# ---- the accumulators' bounds, as fr_matrix.inc states them ----------------------------------------------------------
def chunk_rule(r, words, cap=1024):
    """the chain length T the kernels derive from the modulus's top word: the largest T <= cap with
    T u + 1 < 1 / u, u = (top + 1) / 2^32 an upper bound of r / R"""
    top = r >> (32 * (words - 1))
    assert 0 < top < 1 << 32
    T = 0
    while T < cap and (T + 1) * (top + 1) * (top + 1) + (top + 1) * (1 << 32) < 1 << 64:
        T += 1
    return T


def rule_holds(r, words, T):
    top = r >> (32 * (words - 1))
    return T * (top + 1) * (top + 1) + (top + 1) * (1 << 32) < 1 << 64


def chain_fits(r, words, T):
    """exact integers: T worst products stay in 2 * words words with room for the reduction, and the reduced chain in
    `words` words -- (sum + m r) / R < R for every m < R"""
    R = 1 << (32 * words)
    worst = T * (r - 1) * (r - 1)
    return worst + (R - 1) * r < R * R
