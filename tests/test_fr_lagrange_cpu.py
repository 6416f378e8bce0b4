"""The generator's half of the QAP reduction (amdmsm_fr_domain_lagrange*, amdmsm_fr_matrix_load_transposed and its plan
twin, amdmsm_fr_lincomb_device) as far as a host without a GPU can see it: the symbols are exported and declared, the
closed forms of DESIGN section 24 give the product definition's vector on every small domain of the six fields, the
transposed plan is the plan of the transpose and refuses what the plain one refuses, and the three device entries refuse
what they refuse before they look at the context."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm
import fr_lagrange_model as lm
import fr_matrix_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_fr_domain_lagrange", "amdmsm_fr_domain_lagrange_device", "amdmsm_fr_matrix_load_transposed",
         "amdmsm_plan_fr_matrix_transposed", "amdmsm_fr_lincomb_device")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
CURVES = sorted(fm.CURVES)
PLAN_WORDS = 16
BASE = 0x7f0000000000   # a device address, aligned to anything


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def test_the_symbols_are_exported_and_declared(lib):
    import libff_amd
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(libff_amd.Engine.fr_domain_lagrange) == ["self", "curve", "m", "t", "plain"]
    assert sig(libff_amd.Engine.fr_domain_lagrange_device) == ["self", "curve", "m", "t", "d_out", "plain", "stream"]
    assert sig(libff_amd.Engine.fr_matrix_load_transposed) == sig(libff_amd.Engine.fr_matrix_load)
    assert sig(libff_amd.plan_fr_matrix_transposed) == sig(libff_amd.plan_fr_matrix)
    assert sig(libff_amd.Engine.fr_lincomb_device) == ["self", "curve", "n", "d_vectors", "scalars", "d_out", "plain", "stream"]
    assert "plan_fr_matrix_transposed" in libff_amd.__all__


def domain_sizes(curve, upto=48):
    return [m for m in range(2, upto + 1) if dm.choose(curve, m)[0] == OK and dm.choose(curve, m)[2] == m]


@pytest.mark.parametrize("curve", CURVES)
def test_closed_forms_against_the_definition(curve):
    """every domain size 2 .. 48 (all of them below MNT6's 2-adicity of 17): t random, t = 0, t = x_k; and sum L_j = 1"""
    r = fm.field(curve).r
    rng = random.Random(curve)
    sizes = domain_sizes(curve)
    assert sizes[:6] == [2, 3, 4, 5, 6, 8] and 48 in sizes and 7 not in sizes
    for m in sizes:
        xs = dm.elements(curve, m)
        for t in (rng.randrange(r), 0, xs[0], xs[m - 1], xs[m // 2], xs[rng.randrange(m)]):
            want = lm.lagrange_def(curve, m, t)
            assert lm.lagrange(curve, m, t) == want, (curve, m, t)
            assert sum(want) % r == 1
            if t in xs:
                assert want == [1 if x == t else 0 for x in xs]


def test_closed_forms_at_a_larger_step_domain():
    """m = 2^10 + 1 and 2^10 + 2^6: the closed forms evaluate a polynomial from its values, sum L_j(t) A(x_j) = A(t)"""
    for curve, m in ((0, 1025), (5, (1 << 10) + (1 << 6))):
        r = fm.field(curve).r
        t = random.Random(m).randrange(r)
        L = lm.lagrange(curve, m, t)
        assert sum(L) % r == 1
        a = fm.random_vector(curve, m, seed=3)
        values = dm.transform(curve, a)
        assert sum(x * y for x, y in zip(L, values)) % r == dm.poly_eval(a, t, r)


def test_transpose_and_lincomb_models():
    f = fm.field(0)
    m = mm.random_matrix(f.r, [0, 3, 7, 1, 40, 0, 5], 9, seed=2, nonzero=False)
    t = lm.transpose(m)
    assert (t.n_rows, t.n_cols, t.nnz) == (m.n_cols, m.n_rows, m.nnz)
    assert mm.dense(t, f.r) == [list(col) for col in zip(*mm.dense(m, f.r))]
    assert mm.dense(lm.transpose(t), f.r) == mm.dense(m, f.r)
    for row in t.rows:
        assert [i for i, _ in row] == sorted(i for i, _ in row)
    assert lm.lincomb([[1, 2], [3, 4]], [5, f.r - 1], f.r) == [2, 6]


def matrices(f):
    """(name, Csr): empty columns, repeated pairs, zero coefficients, no rows, no columns' worth of entries, no entries"""
    r = f.r
    yield "classes", mm.Csr([[(2, 1), (0, r - 1), (2, 1)], [], [(4, 7), (1, 0), (6, r - 2)], [(0, 1)], [(4, 0), (4, 0)],
                             [(c % 5, (1, r - 1, 2, 0, 12345)[c % 5]) for c in range(40)]], 9)
    yield "random", mm.random_matrix(r, [random.Random(5).randrange(12) for _ in range(150)], 70, seed=6, nonzero=False)
    yield "long_columns", mm.random_matrix(r, [3] * 500, 4, seed=7, nonzero=False)
    yield "no_rows", mm.Csr([], 5)
    yield "no_columns", mm.Csr([[], [], []], 0)
    yield "no_entries", mm.Csr([[], [], [], []], 6)


@pytest.mark.parametrize("curve", CURVES)
def test_transposed_plan_is_the_plan_of_the_transpose(lib, curve):
    from libff_amd import plan_fr_matrix, plan_fr_matrix_transposed

    f = fm.field(curve)
    for name, m in matrices(f):
        for plain in (False, True):
            off, cols, co = m.arrays(f, plain)
            if not m.n_rows:
                off = np.zeros(0, dtype=np.uint64)
            got = plan_fr_matrix_transposed(curve, off, cols, co, m.n_cols, plain=plain)
            t_off, t_cols, t_co = lm.transpose_arrays(np.array(m.offsets, dtype=np.uint64), cols, co, m.n_cols)
            assert got == plan_fr_matrix(curve, t_off, t_cols, t_co, m.n_rows, plain=plain), (name, plain)
            t = lm.transpose(m)
            assert got["nnz"] == m.nnz and got["longest_row"] == max([0] + mm.row_lengths(t)), name
            assert {k: got[k] for k in ("general", "plus_one", "minus_one", "zero")} == mm.class_counts(m, f.r)


def test_one_column_in_every_row_is_served_by_several_waves(lib, monkeypatch):
    """the column of the constant 1: present in each of 3000 rows, so a row of 3000 entries of the transpose"""
    from libff_amd import plan_fr_matrix, plan_fr_matrix_transposed

    f = fm.field(0)
    rng = random.Random(11)
    rows = [[(0, mm.pick_coeff(rng, f.r) or 1)] + [(1 + rng.randrange(50), rng.randrange(1, f.r)) for _ in range(2)] for _ in range(3000)]
    m = mm.Csr(rows, 51)
    off, cols, co = m.arrays(f, True)
    monkeypatch.setenv("AMDMSM_FR_MATRIX_SPLIT_ROW", "256")
    got = plan_fr_matrix_transposed(0, off, cols, co, m.n_cols, plain=True)
    assert got == plan_fr_matrix(0, *lm.transpose_arrays(off, cols, co, m.n_cols), m.n_rows, plain=True)
    assert got["split_row"] == 256 and got["longest_row"] == 3000 and got["rows_split"] == 1
    assert got["partials"] == -(-3000 // 256) and got["launches"] == 2


def raw_plan(lib, entry, curve, n_rows, n_cols, offsets, cols, coeffs, plain, out=True):
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    words = (ctypes.c_size_t * PLAN_WORDS)()
    return getattr(lib, entry)(curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(offsets), ptr(cols), ptr(coeffs),
                               int(plain), words if out else None)


def raw_load(lib, entry, curve, n_rows, n_cols, offsets, cols, coeffs, plain, out=True):
    """without a context: a refusal of the arrays comes first, the missing context answers BAD_ARG last"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_uint64(77)
    rc = getattr(lib, entry)(None, curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(offsets), ptr(cols), ptr(coeffs),
                             int(plain), ctypes.byref(h) if out else None)
    assert not out or h.value == 0
    return rc


@pytest.mark.parametrize("curve", CURVES)
def test_transposed_plan_and_load_refuse_what_the_plain_ones_refuse(lib, curve):
    f = fm.field(curve)
    m = next(matrices(f))[1]
    off, cols, co = m.arrays(f, True)
    cases = [(curve, m.n_rows, m.n_cols, off, cols, co, True), (17, m.n_rows, m.n_cols, off, cols, co, True)]
    bad = off.copy()
    bad[0] = 1
    cases.append((curve, m.n_rows, m.n_cols, bad, cols, co, True))
    bad = off.copy()
    bad[2] = bad[1] - 1   # a decreasing offset
    cases.append((curve, m.n_rows, m.n_cols, bad, cols, co, True))
    cases.append((curve, m.n_rows, 6, off, cols, co, True))   # column 6 >= n_cols = 6
    for plain in (False, True):   # a coefficient that is r itself, and one above it, in either form
        for v in (f.r, f.r + 5):
            big = m.arrays(f, plain)[2].copy()
            big[3] = np.frombuffer(v.to_bytes(8 * f.limbs, "little"), dtype="<u8")
            cases.append((curve, m.n_rows, m.n_cols, off, cols, big, plain))
    for missing in range(3):   # a null array with work to do
        arrs = [off, cols, co]
        arrs[missing] = None
        cases.append((curve, m.n_rows, m.n_cols, *arrs, True))
    cases += [(curve, 0, 0, None, None, None, True), (curve, 2, 3, np.zeros(3, dtype=np.uint64), None, None, True)]
    cases += [(curve, (1 << 28) + 1, 1, off, cols, co, True), (curve, 1, (1 << 28) + 1, off, cols, co, True),
              (curve, 1, 1, np.array([0, (1 << 31) + 1], dtype=np.uint64), cols, co, True)]
    codes = [raw_plan(lib, "amdmsm_plan_fr_matrix", *c) for c in cases]
    assert codes[:5] == [OK, UNSUPPORTED, BAD_ARG, BAD_ARG, BAD_ARG] and codes[-5:] == [OK, OK, TOO_LARGE, TOO_LARGE, TOO_LARGE]
    assert set(codes[5:-5]) == {BAD_ARG}
    assert [raw_plan(lib, "amdmsm_plan_fr_matrix_transposed", *c) for c in cases] == codes
    assert raw_plan(lib, "amdmsm_plan_fr_matrix_transposed", *cases[0], out=False) == BAD_ARG
    # the loads: the same refusals, and where the plan succeeds the missing context
    loads = [raw_load(lib, "amdmsm_fr_matrix_load", *c) for c in cases]
    assert loads == [c if c else BAD_ARG for c in codes]
    assert [raw_load(lib, "amdmsm_fr_matrix_load_transposed", *c) for c in cases] == loads
    assert raw_load(lib, "amdmsm_fr_matrix_load_transposed", *cases[0], out=False) == BAD_ARG


@pytest.mark.parametrize("curve", [0, 4, 2])   # 8, 10 and 12 words: alignment to 16, 8 and 16 bytes
def test_device_entries_refuse_without_a_context(lib, curve):
    """fake aligned device addresses that nothing reads and no context: every refusal is BAD_ARG (or the code the issue
    names) before the context is looked at, a call that keeps every rule stops at the missing context, and the host
    arrays are as they were"""
    f = fm.field(curve)
    rec = f.limbs * 8
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    N = 8
    good = _Opts(ctypes.sizeof(_Opts), 0, 0, 1, 1, 0, None)
    o = ctypes.byref(good)
    wrong = ctypes.byref(_Opts(ctypes.sizeof(_Opts) - 4, 0, 0, 1, 1, 0, None))
    host = np.ones((8, f.limbs), dtype=np.uint64)            # plain records: 1 .. and room for a host result
    host[:4] = f.records([5, 0, f.r - 1, 7], True)
    too_big = np.frombuffer(f.r.to_bytes(rec, "little"), dtype="<u8").copy()
    hp = lambda k=0: vp(host.ctypes.data + k * rec)
    A, B, C, D, OUT = (BASE + i * 4 * N * rec for i in range(5))

    lag_d = lambda m, t, dst, opts=o, c=curve: lib.amdmsm_fr_domain_lagrange_device(None, c, sz(m), t, opts, vp(dst))
    lag_h = lambda m, t, dst, opts=o, c=curve: lib.amdmsm_fr_domain_lagrange(None, c, sz(m), t, opts, dst)

    def lin(n, vecs, scalars, dst, opts=o, c=curve, k=None):
        ptrs = (ctypes.c_void_p * 4)(*[vp(v) for v in vecs])
        return lib.amdmsm_fr_lincomb_device(None, c, sz(n), len(vecs) if k is None else k, ptrs, scalars, opts, vp(dst))

    before = host.copy()
    assert lag_d(N, hp(), OUT, c=17) == UNSUPPORTED and lag_h(N, hp(), hp(4), c=17) == UNSUPPORTED
    assert lag_d((1 << 28) + 1, hp(), OUT) == TOO_LARGE and lag_h((1 << 28) + 1, hp(), hp(4)) == TOO_LARGE
    assert lag_d((1 << 18) + 1, hp(), OUT, c=5) == UNSUPPORTED   # MNT6: a domain left out
    refused = [
        lag_d(7, hp(), OUT), lag_d(11, hp(), OUT), lag_d(1, hp(), OUT), lag_d(0, hp(), OUT),   # no domain size; m < 2
        lag_d(N, None, OUT), lag_d(N, hp(), 0), lag_d(N, vp(too_big.ctypes.data), OUT),        # null t, null output, t = r
        lag_d(N, hp(), OUT + 4), lag_d(N, hp(), OUT, wrong),
        lag_h(7, hp(), hp(4)), lag_h(1, hp(), hp(4)), lag_h(N, None, hp(4)), lag_h(N, hp(), None),
        lag_h(N, vp(too_big.ctypes.data), hp(4)), lag_h(N, hp(), hp(4), wrong),
        lin(N, [A], hp(), OUT, k=0), lin(N, [A, B, C, D], hp(), OUT, k=5), lin(N, [A], hp(), OUT, wrong),
        lin(N, [A, 0], hp(), OUT), lin(N, [A], hp(), 0), lin(N, [A], None, OUT),               # null vector, output, scalars
        lin(N, [A], vp(too_big.ctypes.data), OUT),                                             # a scalar that is r
        lin(N, [A + 4], hp(), OUT), lin(N, [A, B + 4], hp(), OUT), lin(N, [A], hp(), OUT + 4),
        lin(N, [A, B], hp(), A + rec), lin(N, [A, B], hp(), B - rec), lin(N, [A, B, C, D], hp(), D + (N - 1) * rec),
    ]
    assert refused == [BAD_ARG] * len(refused)
    assert lin((1 << 28) + 1, [A], hp(), OUT) == TOO_LARGE and lin(N, [A], hp(), OUT, c=17) == UNSUPPORTED
    kept = [
        lag_d(N, hp(), OUT), lag_d(2, hp(1), OUT), lag_d(3, hp(2), OUT), lag_d((1 << 10) + 1, hp(), OUT),   # t = 5, 0, r - 1
        lag_h(N, hp(), hp(4)),
        lin(N, [A], hp(), OUT), lin(N, [A, B, C, D], hp(), OUT), lin(N, [A, B], hp(), A), lin(N, [A, B], hp(), B),
        lin(N, [A, B], hp(), A + N * rec), lin(N, [A, A], hp(), A), lin(0, [A + 4, 0], hp(), 0),
    ]
    assert kept == [BAD_ARG] * len(kept)
    assert (host == before).all()
