"""Integer model of what the generator's half of the QAP reduction needs on top of fr_domain_model: the Lagrange vector
of a domain at a point -- by the product definition and by the closed forms of DESIGN section 24 -- the transpose of a
CSR matrix, and a linear combination of vectors.  Python integers only; nothing here knows of tables, sweeps or batch
inversion.  transpose_arrays does to the numpy arrays of a load what transpose does to the model's rows."""
import numpy as np

import fr_domain_model as dm
import fr_fft_model as fm
from fr_matrix_model import Csr


def lagrange_def(curve, m, t):
    """L_j(t) = prod over k != j of (t - x_k) / (x_j - x_k), every j: O(m^2), for small m"""
    r = fm.field(curve).r
    xs = dm.elements(curve, m)
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num = num * (t - xk) % r
                den = den * (xj - xk) % r
        out.append(num * pow(den, -1, r) % r)
    return out


def denominators(curve, m, t):
    """1 / L_j(t) by the closed forms, Z(t) != 0:
        basic            (t / x_j - 1) m / Z
        step, j < B      (t / x_j - 1) B (rho^(j mod K) - w^S) / Z,  rho = w^(2 S), K = B / S
        step, j >= B     (t / x_j - 1) (-2 S w^S) / Z"""
    f = fm.field(curve)
    r = f.r
    B, S = dm.shape(curve, m)
    xs = dm.elements(curve, m)
    zi = pow(dm.vanishing(curve, m, t), -1, r)
    lead = [(t * pow(x, -1, r) - 1) % r for x in xs]
    if not S:
        return [v * m % r * zi % r for v in lead]
    w = f.root(2 * B)
    ws, K = pow(w, S, r), B // S
    rho = ws * ws % r
    head = [B * (pow(rho, k, r) - ws) % r * zi % r for k in range(K)]
    tail = -2 * S * ws % r * zi % r
    return [lead[j] * (head[j % K] if j < B else tail) % r for j in range(m)]


def lagrange(curve, m, t):
    """the same vector by the closed forms; on a point of the domain the unit vector"""
    r = fm.field(curve).r
    if dm.vanishing(curve, m, t) == 0:
        return [1 if x == t else 0 for x in dm.elements(curve, m)]
    den = denominators(curve, m, t)
    # one inversion for all of them, as a reader would do it by hand
    prefix, acc = [], 1
    for d in den:
        prefix.append(acc)
        acc = acc * d % r
    inv = pow(acc, -1, r)
    out = [0] * m
    for j in range(m - 1, -1, -1):
        out[j] = inv * prefix[j] % r
        inv = inv * den[j] % r
    return out


def lagrange_at(curve, m, t, j):
    """L_j(t) alone by the closed forms, Z(t) != 0: for samples of a large domain"""
    f = fm.field(curve)
    r = f.r
    B, S = dm.shape(curve, m)
    zi = pow(dm.vanishing(curve, m, t), -1, r)
    if not S:
        x, fac = pow(f.root(m), j, r), m
    else:
        w = f.root(2 * B)
        ws = pow(w, S, r)
        if j < B:
            x, fac = pow(w, 2 * j, r), B * (pow(ws, 2 * (j % (B // S)), r) - ws)
        else:
            x, fac = w * pow(f.root(S), j - B, r) % r, -2 * S * ws
    return pow((t * pow(x, -1, r) - 1) * fac % r * zi % r, -1, r)


def transpose(csr):
    """the CSR of the transpose: row c lists (i, coeff) for the entries (i, c), in ascending i, those of one row in the
    order given; zero coefficients stay"""
    rows = [[] for _ in range(csr.n_cols)]
    for i, row in enumerate(csr.rows):
        for c, v in row:
            rows[c].append((i, v))
    return Csr(rows, csr.n_rows)


def transpose_arrays(offsets, cols, coeffs, n_cols):
    """the CSR arrays of the transpose from those of the matrix, by a stable sort of the entries on the column"""
    n_rows = max(0, len(offsets) - 1)
    rows = np.repeat(np.arange(n_rows, dtype=np.uint32), np.diff(np.asarray(offsets, dtype=np.int64)))
    order = np.argsort(cols, kind="stable")
    t_off = np.zeros(n_cols + 1, dtype=np.uint64)
    t_off[1:] = np.cumsum(np.bincount(np.asarray(cols, dtype=np.int64), minlength=n_cols))
    return t_off, rows[order], coeffs[order]


def lincomb(vectors, scalars, r):
    """out[i] = sum_j scalars[j] * vectors[j][i]"""
    assert len(vectors) == len(scalars) and vectors
    return [sum(s * v[i] for s, v in zip(scalars, vectors)) % r for i in range(len(vectors[0]))]
