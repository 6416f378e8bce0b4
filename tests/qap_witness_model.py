"""Integer model of the R1CS-to-QAP witness map that Engine.qap_witness_map computes: with aA, aB, aC the products of the
three constraint matrices with the assignment z, zero-filled to the m points of the domain, A, B, C the polynomials of
degree < m with those values on the domain and Z its vanishing polynomial, the m + 1 coefficients of the H with

    (A + d1 Z) (B + d2 Z) - (C + d3 Z) = H Z,      H = (A B - C) / Z + d2 A + d1 B + d1 d2 Z - d3.

Interpolation is fr_domain_model's, the division an exact long division by the dense Z.  Python integers only; nothing
here knows of cosets, transforms on the device or the order of the library's calls."""
import random

import fr_domain_model as dm
import fr_fft_model as fm
import fr_matrix_model as mm


def dense_z(curve, m):
    z = [0] * (m + 1)
    for i, coef in dm.z_terms(curve, m):
        z[i] = (z[i] + coef) % fm.field(curve).r
    return z


def poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % r for v in out]


def divide_exactly(num, z, r):
    """num / z for a monic z that divides num; AssertionError where a remainder is left"""
    m = len(z) - 1
    assert z[m] == 1
    num = list(num)
    q = [0] * max(len(num) - m, 0)
    terms = [(i, c) for i, c in enumerate(z[:m]) if c]
    for k in range(len(num) - 1, m - 1, -1):
        c = num[k] % r
        q[k - m] = c
        if c:
            for i, zc in terms:
                num[k - m + i] -= c * zc
    assert all(v % r == 0 for v in num[:m]), "Z does not divide A B - C: the assignment does not satisfy the system"
    return q


def polynomials(curve, a, b, c, z, m):
    """A, B, C: the coefficients of the interpolants of the three applies, zero-filled to m"""
    r = fm.field(curve).r
    return [dm.interpolate(curve, mm.apply(mat, z, r, n_out=m)) for mat in (a, b, c)]


def witness_map(curve, a, b, c, z, m, blind=None):
    """the m + 1 coefficients of H; blind: (d1, d2, d3) or None"""
    r = fm.field(curve).r
    A, B, C = polynomials(curve, a, b, c, z, m)
    num = poly_mul(A, B, r)
    for i, x in enumerate(C):
        num[i] = (num[i] - x) % r
    q = divide_exactly(num, dense_z(curve, m), r)
    h = q + [0] * (m + 1 - len(q))
    if blind is not None:
        d1, d2, d3 = blind
        for i in range(m):
            h[i] = (h[i] + d2 * A[i] + d1 * B[i]) % r
        for i, zc in enumerate(dense_z(curve, m)):
            h[i] = (h[i] + d1 * d2 * zc) % r
        h[0] = (h[0] - d3) % r
    return h


def identity_holds(curve, a, b, c, z, m, h, blind=None):
    """(A + d1 Z)(B + d2 Z) - (C + d3 Z) == H Z, coefficient by coefficient"""
    r = fm.field(curve).r
    d1, d2, d3 = blind or (0, 0, 0)
    zd = dense_z(curve, m)
    A, B, C = ([(x + d * zc) % r for x, zc in zip(p + [0], zd)] for p, d in zip(polynomials(curve, a, b, c, z, m), (d1, d2, d3)))
    lhs = poly_mul(A, B, r)
    for i, x in enumerate(C):
        lhs[i] = (lhs[i] - x) % r
    rhs = poly_mul(h, zd, r)
    n = max(len(lhs), len(rhs))
    return [v for v in lhs + [0] * (n - len(lhs))] == [v for v in rhs + [0] * (n - len(rhs))]


_systems = {}


def random_system(curve, n_rows, n_cols, seed=0):
    """(A, B, C, z): a satisfied system of n_rows constraints over n_cols variables, z[0] = 1, the constant column in
    every row of every matrix; computed once and never changed"""
    key = (curve, n_rows, n_cols, seed)
    if key not in _systems:
        r = fm.field(curve).r
        rng = random.Random(7919 * curve + 101 * n_rows + seed)
        z = [1] + [mm.pick_x(rng, r) for _ in range(n_cols - 1)]
        rows = {k: [] for k in "abc"}
        for _ in range(n_rows):
            dot = {}
            for k in "abc":
                row = [(0, mm.pick_coeff(rng, r) or 1)]
                row += [(rng.randrange(1, n_cols), mm.pick_coeff(rng, r)) for _ in range(rng.randrange(0, 4))]
                rows[k].append(row)
                dot[k] = sum(v * z[col] for col, v in row) % r
            # the constant column of C makes the row hold: <C, z> = <A, z> <B, z>
            col0, v0 = rows["c"][-1][0]
            rows["c"][-1][0] = (col0, (v0 + dot["a"] * dot["b"] - dot["c"]) % r)
        _systems[key] = tuple(mm.Csr(rows[k], n_cols) for k in "abc") + (z,)
    return _systems[key]
