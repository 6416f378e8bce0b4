"""Integer model of the evaluation domains over Fr that the fr_domain entries serve: libfqfft's choice between the basic
radix-2 domain and the step radix-2 domain of m = B + S points (B, S powers of two, S < B), the elements, the vanishing
polynomial, the transform (evaluation at g x_j, in the order of the elements), its inverse (interpolation) and the
division by Z on a coset.  Python integers only, on top of fr_fft_model; nothing here knows of folds, partial sums or
passes.  Restated from the definitions of DESIGN section 22, not from libfqfft's code."""
import fr_fft_model as fm

BASIC, STEP = 0, 1
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
MAX_M = 1 << 28


def log2_ceil(n):
    return (n - 1).bit_length() if n > 1 else 0


def choose(curve, min_size):
    """(code, kind, m, B, S, log2 of omega's order): what amdmsm_fr_domain answers; kind .. are None unless code is OK"""
    s = fm.TWO_ADICITY[curve]
    none = (None,) * 5
    if min_size < 2:
        return (BAD_ARG,) + none
    big = 1 << (log2_ceil(min_size) - 1)
    small = min_size - big
    rounded = 1 << log2_ceil(small)
    if min_size & (min_size - 1) == 0:
        kind, m = BASIC, min_size
    elif small & (small - 1) == 0:
        kind, m = STEP, min_size
    elif (big + rounded) & (big + rounded - 1) == 0:
        kind, m = BASIC, big + rounded
    else:
        kind, m = STEP, big + rounded
    if m > MAX_M:
        return (TOO_LARGE,) + none
    if kind == BASIC:
        if log2_ceil(m) > s:
            return (UNSUPPORTED,) + none
        return OK, BASIC, m, m, 0, log2_ceil(m)
    B = 1 << (log2_ceil(m) - 1)
    if log2_ceil(2 * B) > s:
        return (UNSUPPORTED,) + none
    return OK, STEP, m, B, m - B, log2_ceil(2 * B)


def shape(curve, m):
    """(B, S) of the domain of exactly m points; S = 0: basic"""
    code, kind, mm, B, S, _ = choose(curve, m)
    assert code == OK and mm == m, (curve, m)
    return B, S


def elements(curve, m):
    f = fm.field(curve)
    B, S = shape(curve, m)
    if not S:
        w = f.root(m)
        return [pow(w, j, f.r) for j in range(m)]
    w, sg = f.root(2 * B), f.root(S)
    return [pow(w, 2 * j, f.r) for j in range(B)] + [w * pow(sg, j, f.r) % f.r for j in range(S)]


def z_terms(curve, m):
    """Z as [(index, coefficient)], the highest index first"""
    f = fm.field(curve)
    B, S = shape(curve, m)
    if not S:
        return [(m, 1), (0, f.r - 1)]
    ws = pow(f.root(2 * B), S, f.r)
    return [(B + S, 1), (B, f.r - ws), (S, f.r - 1), (0, ws)]


def vanishing(curve, m, t):
    f = fm.field(curve)
    B, S = shape(curve, m)
    if not S:
        return (pow(t, m, f.r) - 1) % f.r
    return (pow(t, B, f.r) - 1) * (pow(t, S, f.r) - pow(f.root(2 * B), S, f.r)) % f.r


def poly_eval(coeffs, t, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * t + c) % r
    return acc


def transform_horner(curve, a, g=1):
    """out[j] = A(g x_j) by Horner's rule at every point: m <= 96"""
    f = fm.field(curve)
    assert len(a) <= 96
    return [poly_eval(a, g * x % f.r, f.r) for x in elements(curve, len(a))]


def transform(curve, a, g=1):
    """the same values through the decomposition into a size-B and a size-S radix-2 transform (fr_fft_model.fft)"""
    f = fm.field(curve)
    r, m = f.r, len(a)
    B, S = shape(curve, m)
    if not S:
        return fm.fft(a, f.root(m), r, pre=g)
    w = f.root(2 * B)
    ap = [a[i] * pow(g, i, r) % r for i in range(m)]
    c = [(ap[i] + ap[B + i]) % r if i < S else ap[i] for i in range(B)]
    d = [pow(w, i, r) * ((ap[i] - ap[B + i]) if i < S else ap[i]) % r for i in range(B)]
    e = [sum(d[i::S]) % r for i in range(S)]
    return fm.fft(c, w * w % r, r) + fm.fft(e, f.root(S), r)


def interpolate(curve, values, g=1):
    """the coefficients of the A of degree < m with A(g x_j) = values[j]: the inverse of transform"""
    f = fm.field(curve)
    r, m = f.r, len(values)
    B, S = shape(curve, m)
    gi = pow(g, -1, r)
    if not S:
        return fm.fft(values, pow(f.root(m), -1, r), r, post=gi, scale=pow(m, -1, r))
    w = f.root(2 * B)
    wi, K, half = pow(w, -1, r), B // S, pow(2, -1, r)
    u0 = fm.fft(values[:B], wi * wi % r, r, scale=pow(B, -1, r))
    u1 = fm.fft(values[B:], pow(f.root(S), -1, r), r, scale=pow(S, -1, r))
    a = list(u0) + [0] * S
    for i in range(S):
        t = sum(pow(w, i + j * S, r) * u0[i + j * S] for j in range(1, K)) % r
        v = pow(wi, i, r) * (u1[i] - t) % r
        a[i], a[B + i] = (u0[i] + v) * half % r, (u0[i] - v) * half % r
    return [a[i] * pow(gi, i, r) % r for i in range(m)]


def divide_by_z(curve, values, g):
    """out[j] = values[j] / Z(g x_j); None where some denominator is 0"""
    f = fm.field(curve)
    m = len(values)
    den = [vanishing(curve, m, g * x % f.r) for x in elements(curve, m)]
    if not all(den):
        return None
    return [v * pow(d, -1, f.r) % f.r for v, d in zip(values, den)]
