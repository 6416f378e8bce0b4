"""The generator's half of the QAP reduction on the device: the Lagrange vector of a domain at a point
(Engine.fr_domain_lagrange and its device form) against the product definition and the closed forms of
tests/fr_lagrange_model.py, the transposed sparse map (Engine.fr_matrix_load_transposed) against the transpose built with
integers and with numpy, the linear combination of resident vectors (Engine.fr_lincomb_device), and the three together:
At, Bt, Ct and a key vector of a small constraint system from t onwards."""
import ctypes
import random

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm
import fr_lagrange_model as lm
import fr_matrix_model as mm
from fr_dev import BAD_ARG, SENTINEL, TOO_LARGE, UNSUPPORTED, Dev, at, env_path, hip_runtime, poly_eval

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402

SIX = [pytest.param(c, id=n) for c, n in fm.CURVES.items()]
_expected = {}


def point(curve, m, seed=0):
    return random.Random(1000 * m + curve + seed).randrange(fm.field(curve).r)


def expected(curve, m, t):
    """the closed-form vector, computed once per (curve, m, t)"""
    key = (curve, m, t)
    if key not in _expected:
        _expected[key] = lm.lagrange(curve, m, t)
    return _expected[key]


def domain_sizes(curve, upto):
    return [m for m in range(2, upto + 1) if dm.choose(curve, m)[0] == 0 and dm.choose(curve, m)[2] == m]


@pytest.mark.parametrize("curve", SIX)
def test_every_small_domain_against_the_definition(engine, curve):
    """m = 2 .. 24, the product definition itself, both record forms"""
    f = fm.field(curve)
    sizes = domain_sizes(curve, 24)
    assert sizes == [2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 17, 18, 20, 24]
    for m in sizes:
        t = point(curve, m)
        want = lm.lagrange_def(curve, m, t)
        for plain in (False, True):
            got = engine.fr_domain_lagrange(curve, m, t, plain=plain)
            assert f.ints(got, plain) == want, (curve, m, plain)


@pytest.mark.parametrize("m", [(1 << 4) + 1, (1 << 10) + 1, 3 << 9, (1 << 10) + (1 << 3), (1 << 12) + (1 << 4), 1 << 13],
                         ids=["S1_17", "S1_1025", "K2", "K128_S8", "several_workgroups_and_tiles", "basic_2p13"])
def test_step_shapes_against_the_closed_forms(engine, m):
    """S = 1 with K = B; K = 2; a K-table shorter than a wave's columns; several workgroups and inversion tiles; a basic
    domain"""
    for curve, plain in ((0, False), (4, True)):
        f = fm.field(curve)
        t = point(curve, m)
        got = f.ints(engine.fr_domain_lagrange(curve, m, t, plain=plain), plain)
        assert got == expected(curve, m, t), (curve, m)
        assert sum(got) % f.r == 1


def test_large_domain_sampled(engine):
    """2^17 + 2^9: 64 records against the closed form of each, and the whole vector sums to 1"""
    curve, m = 0, (1 << 17) + (1 << 9)
    f = fm.field(curve)
    t = point(curve, m)
    got = engine.fr_domain_lagrange(curve, m, t, plain=True)
    rng = random.Random(3)
    B = 1 << 17
    picks = [0, 1, B - 1, B, B + 1, m - 1, B // 2, B // 2 + 1] + [rng.randrange(m) for _ in range(56)]
    assert f.ints(got[picks], True) == [lm.lagrange_at(curve, m, t, j) for j in picks]
    assert sum(f.ints(got, True)) % f.r == 1


@pytest.mark.parametrize("m", [24, (1 << 10) + (1 << 3), 16])
def test_points_of_the_domain_give_unit_vectors(engine, m):
    """Z(t) = 0: x_0, x_(B-1), x_B (the first point of the tail), x_(m-1), exactly e_k in both forms; nothing is inverted"""
    for curve in (0, 4):
        f = fm.field(curve)
        B = dm.shape(curve, m)[0]
        for k in sorted({0, B - 1, B % m, m - 1}):
            t = libff_amd.fr_domain_element(curve, m, k)
            assert libff_amd.fr_domain_vanishing(curve, m, t) == 0
            unit = [0] * m
            unit[k] = 1
            for plain in (False, True):
                got = engine.fr_domain_lagrange(curve, m, t, plain=plain)
                assert (got == f.records(unit, plain)).all(), (curve, m, k, plain)


@pytest.mark.parametrize("m", [6, 16, (1 << 10) + (1 << 3)])
def test_t_is_zero(engine, m):
    for curve, plain in ((0, True), (3, False)):
        f = fm.field(curve)
        got = f.ints(engine.fr_domain_lagrange(curve, m, 0, plain=plain), plain)
        assert got == expected(curve, m, 0)
        if m <= 16:
            assert got == lm.lagrange_def(curve, m, 0)


@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(5, id="mnt6")])
def test_device_entry_between_sentinels_and_on_a_stream(engine, curve):
    f = fm.field(curve)
    rec = f.limbs * 8
    m = (1 << 12) + (1 << 4)
    t = point(curve, m)
    want = f.records(expected(curve, m, t), False)
    hip = hip_runtime()
    with Dev(engine) as d:
        blank = np.full((m + 4, f.limbs), SENTINEL, dtype=np.uint64)
        d_out = d.up(blank)
        engine.fr_domain_lagrange_device(curve, m, t, at(d_out, 2 * rec))
        got = d.down(d_out, blank.shape)
        assert (got[2:-2] == want).all() and (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        # the unit vector takes the other path of the same launcher
        engine.fr_domain_lagrange_device(curve, m, libff_amd.fr_domain_element(curve, m, m - 1), at(d_out, 2 * rec), plain=True)
        got = d.down(d_out, blank.shape)
        assert (got[2:-3] == 0).all() and got[-3, 0] == 1 and (got[-3, 1:] == 0).all()
        assert (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        # a stream of the caller's
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        try:
            d_two = d.up(blank)
            engine.fr_domain_lagrange_device(curve, m, t, at(d_two, 2 * rec), stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
        finally:
            assert hip.hipStreamDestroy(stream) == 0
        got = d.down(d_two, blank.shape)
        assert (got[2:-2] == want).all() and (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()


def test_the_naive_inversion_gives_the_same_bytes(engine):
    m = (1 << 12) + (1 << 4)
    for curve, plain in ((0, False), (2, True)):
        t = point(curve, m)
        tiled = engine.fr_domain_lagrange(curve, m, t, plain=plain)
        with env_path("AMDMSM_FR_SCAN_NAIVE", True):
            naive = engine.fr_domain_lagrange(curve, m, t, plain=plain)
        assert (tiled == naive).all() and fm.field(curve).ints(tiled[:8], plain) == expected(curve, m, t)[:8]


def test_lagrange_refusals_with_a_context(engine):
    f = fm.field(0)
    rec = f.limbs * 8
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    with Dev(engine) as d:
        blank = np.full((24, f.limbs), SENTINEL, dtype=np.uint64)
        d_buf = d.up(blank)
        with pytest.raises(libff_amd.AmdMsmError, match=r"m = 7 .* 8 ") as e:
            engine.fr_domain_lagrange_device(0, 7, 5, d_buf)
        assert e.value.code == BAD_ARG
        with pytest.raises(libff_amd.AmdMsmError, match=r"m = 11 .* 12 "):
            engine.fr_domain_lagrange_device(0, 11, 5, d_buf)
        with pytest.raises(libff_amd.AmdMsmError, match="at least 2 points") as e:
            engine.fr_domain_lagrange_device(0, 1, 5, d_buf)
        assert e.value.code == BAD_ARG
        with pytest.raises(libff_amd.AmdMsmError, match="2\\^28") as e:
            engine.fr_domain_lagrange_device(0, (1 << 28) + 1, 5, d_buf)
        assert e.value.code == TOO_LARGE
        with pytest.raises(libff_amd.AmdMsmError, match="geometric") as e:
            engine.fr_domain_lagrange_device(5, (1 << 17) + 1, 5, d_buf)
        assert e.value.code == UNSUPPORTED
        with pytest.raises(libff_amd.AmdMsmError, match="extended") as e:
            engine.fr_domain_lagrange_device(5, 1 << 18, 5, d_buf)
        assert e.value.code == UNSUPPORTED
        five, o = f.records([5], False), engine._opts()
        raw = lambda curve: engine.lib.amdmsm_fr_domain_lagrange_device(engine.h, curve, ctypes.c_size_t(8), five.ctypes.data_as(ctypes.c_void_p),
                                                                       ctypes.byref(o), d_buf)
        assert raw(17) == UNSUPPORTED and "unknown curve" in err()
        with pytest.raises(libff_amd.AmdMsmError, match="d_out: not aligned") as e:
            engine.fr_domain_lagrange_device(0, 8, 5, at(d_buf, 4))
        assert e.value.code == BAD_ARG
        with pytest.raises(libff_amd.AmdMsmError, match="output: null") as e:
            engine.fr_domain_lagrange_device(0, 8, 5, None)
        assert e.value.code == BAD_ARG
        too_big = np.frombuffer(f.r.to_bytes(rec, "little"), dtype="<u8").astype(np.uint64)
        with pytest.raises(libff_amd.AmdMsmError, match="t: not below r") as e:
            engine.fr_domain_lagrange_device(0, 8, too_big, d_buf)
        assert e.value.code == BAD_ARG
        o = engine._opts()
        assert engine.lib.amdmsm_fr_domain_lagrange_device(engine.h, 0, ctypes.c_size_t(8), None, ctypes.byref(o), d_buf) == BAD_ARG
        assert "t: null" in err()
        o.struct_size -= 4
        assert engine.lib.amdmsm_fr_domain_lagrange_device(engine.h, 0, ctypes.c_size_t(8), None, ctypes.byref(o), d_buf) == BAD_ARG
        assert "struct_size" in err()
        assert (d.down(d_buf, blank.shape) == SENTINEL).all()


def test_lagrange_phases(engine):
    """[0] the tables, [1] the kernels, [2] the download of the host entry alone; a ticket per call"""
    curve, m = 1, (1 << 11) + (1 << 7)
    f = fm.field(curve)
    t = point(curve, m)
    want = f.records(expected(curve, m, t), False)
    with Dev(engine) as d:
        d_out = d.buf(m * f.limbs * 8)
        try:
            engine.set_timing(True)
            last = engine.last_timing_ticket()
            assert (engine.fr_domain_lagrange(curve, m, t) == want).all()
            ticket = engine.last_timing_ticket()
            ph = engine.get_timings(ticket=ticket)
            print("host", ph)
            assert ticket != last
            assert ph["count_ms"] > 0 and ph["scatter_ms"] > 0 and ph["accumulate_ms"] > 0 and ph["total_ms"] >= ph["scatter_ms"]
            last = ticket
            engine.fr_domain_lagrange_device(curve, m, t, d_out)
            assert (d.down(d_out, (m, f.limbs)) == want).all()
            ticket = engine.last_timing_ticket()
            ph = engine.get_timings(ticket=ticket)
            print("device", ph)
            assert ticket != last and ph["scatter_ms"] > 0 and ph["count_ms"] >= 0 and ph["accumulate_ms"] == 0
        finally:
            engine.set_timing(False)
        assert (engine.fr_domain_lagrange(curve, m, t) == want).all()


def test_evaluation_form_against_the_inverse_transform(engine):
    """sum_j L_j(t) values[j] = A(t), A the coefficients the library's own inverse transform gives"""
    m = (1 << 10) + (1 << 6)
    for curve, plain in ((0, False), (4, True)):
        f = fm.field(curve)
        t = point(curve, m, seed=1)
        values = fm.random_vector(curve, m, seed=8)
        coeffs = f.ints(engine.fr_domain_fft(curve, f.records(values, plain), inverse=True, plain=plain), plain)
        L = f.ints(engine.fr_domain_lagrange(curve, m, t, plain=plain), plain)
        assert sum(x * y for x, y in zip(L, values)) % f.r == poly_eval(coeffs, t, f.r)


# ---- the transposed map ------------------------------------------------------------------------------------------------
def r1cs_like(f, seed, rows=120, cols=37):
    """rows of 0 .. 9 entries over few columns: repeated pairs, zero coefficients, an empty column (the last)"""
    lengths = [random.Random(seed).randrange(10) for _ in range(rows)]
    m = mm.random_matrix(f.r, lengths, cols - 1, seed=seed, nonzero=False)
    return mm.Csr(m.rows, cols)


@pytest.mark.parametrize("naive", [False, True], ids=["resident", "naive"])
def test_transposed_apply(engine, naive):
    """against apply(transpose(M), u) in integers, bit for bit against a handle loaded from the transpose numpy builds,
    and zeros up to n_out"""
    for curve, plain in ((0, False), (4, True), (2, False)):
        f = fm.field(curve)
        m = r1cs_like(f, seed=20 + curve)
        off, cols, co = m.arrays(f, plain)
        u = mm.random_x(f.r, m.n_rows + 3, seed=curve)
        want = mm.apply(lm.transpose(m), u, f.r, n_out=m.n_cols + 5)
        assert any(want[:m.n_cols]) and want[m.n_cols - 1] == 0
        with env_path("AMDMSM_FR_MATRIX_NAIVE", naive):
            mt = engine.fr_matrix_load_transposed(curve, off, cols, co, m.n_cols, plain=plain)
            ref = engine.fr_matrix_load(curve, *lm.transpose_arrays(off, cols, co, m.n_cols), m.n_rows, plain=plain)
        with mt, ref:
            assert (mt.n_rows, mt.n_cols) == (m.n_cols, m.n_rows)
            got = engine.fr_matrix_apply(mt, f.records(u, plain), n_out=m.n_cols + 5, plain=plain)
            assert f.ints(got, plain) == want, (curve, naive)
            assert (got == engine.fr_matrix_apply(ref, f.records(u, plain), n_out=m.n_cols + 5, plain=plain)).all()


def test_transposed_empty_shapes(engine):
    f = fm.field(0)
    none = np.zeros((0, f.limbs), dtype=np.uint64)
    with engine.fr_matrix_load_transposed(0, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), none, 5) as mt:
        assert (mt.n_rows, mt.n_cols) == (5, 0)
        assert (engine.fr_matrix_apply(mt, none, n_out=7) == 0).all()
    with engine.fr_matrix_load_transposed(0, np.zeros(4, dtype=np.uint64), np.zeros(0, dtype=np.uint32), none, 0) as mt:
        assert (mt.n_rows, mt.n_cols) == (0, 3)
        assert engine.fr_matrix_apply(mt, f.records([1, 2, 3], False)).shape == (0, f.limbs)


def test_one_column_in_every_row(engine, monkeypatch):
    """the column of the constant 1 in each of 3000 constraints: a row of the transpose that several waves serve"""
    f = fm.field(0)
    rng = random.Random(11)
    rows = [[(0, mm.pick_coeff(rng, f.r) or 1)] + [(1 + rng.randrange(50), rng.randrange(1, f.r)) for _ in range(2)] for _ in range(3000)]
    m = mm.Csr(rows, 51)
    off, cols, co = m.arrays(f, False)
    u = mm.random_x(f.r, m.n_rows, seed=4)
    want = mm.apply(lm.transpose(m), u, f.r)
    monkeypatch.setenv("AMDMSM_FR_MATRIX_SPLIT_ROW", "256")
    assert libff_amd.plan_fr_matrix_transposed(0, off, cols, co, m.n_cols)["rows_split"] == 1
    with engine.fr_matrix_load_transposed(0, off, cols, co, m.n_cols) as mt:
        assert f.ints(engine.fr_matrix_apply(mt, f.records(u, False)), False) == want
    monkeypatch.delenv("AMDMSM_FR_MATRIX_SPLIT_ROW")
    with engine.fr_matrix_load_transposed(0, off, cols, co, m.n_cols) as mt:
        assert f.ints(engine.fr_matrix_apply(mt, f.records(u, False)), False) == want


def test_transposed_load_refusals_name_the_matrix_as_given(engine):
    f = fm.field(0)
    m = r1cs_like(f, seed=1, rows=12, cols=9)
    off, cols, co = m.arrays(f, True)
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    k = 5
    bad = co.copy()
    bad[k] = np.frombuffer(f.r.to_bytes(8 * f.limbs, "little"), dtype="<u8")
    bad[m.nnz - 1] = bad[k]
    messages = []
    for load in (engine.fr_matrix_load, engine.fr_matrix_load_transposed):
        with pytest.raises(libff_amd.AmdMsmError, match=f"entry {k}: coefficient >= r"):
            load(0, off, cols, bad, m.n_cols, plain=True)
        with pytest.raises(libff_amd.AmdMsmError, match="column"):
            load(0, off, cols, co, max(m.cols), plain=True)
        messages.append(err())
    assert messages[0] == messages[1]


# ---- linear combinations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, (1 << 12) + 3])
def test_lincomb(engine, n):
    """k = 1 .. 4, out of place between sentinels and in place on each operand, both record forms"""
    for curve, plain in ((0, False), (4, True), (2, False), (3, True)):
        f = fm.field(curve)
        rec = f.limbs * 8
        rng = random.Random(n + curve)
        vecs = [fm.random_vector(curve, n, seed=30 + j) for j in range(4)]
        recs = [f.records(v, plain) for v in vecs]
        scalars = [rng.randrange(f.r), 1, f.r - 1, 0]
        rng.shuffle(scalars)
        with Dev(engine) as d:
            for k in range(1, 5):
                want = f.records(lm.lincomb(vecs[:k], scalars[:k], f.r), plain)
                bufs = [d.up(x) for x in recs[:k]]
                blank = np.full((n + 2, f.limbs), SENTINEL, dtype=np.uint64)
                d_out = d.up(blank)
                engine.fr_lincomb_device(curve, n, bufs, scalars[:k], at(d_out, rec), plain=plain)
                got = d.down(d_out, blank.shape)
                assert (got[1:-1] == want).all() and (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (curve, k)
                for j in range(k):   # in place on operand j, the others as they were
                    engine.fr_lincomb_device(curve, n, bufs, scalars[:k], bufs[j], plain=plain)
                    assert (d.down(bufs[j], (n, f.limbs)) == want).all(), (curve, k, j)
                    engine.h2d(bufs[j], recs[j])


def test_lincomb_rules_with_a_context(engine):
    f = fm.field(0)
    rec = f.limbs * 8
    n = 16
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    with Dev(engine) as d:
        a = f.records(fm.random_vector(0, 2 * n, seed=1), False)
        d_a, d_b = d.up(a), d.up(a)
        blank = np.full((n, f.limbs), SENTINEL, dtype=np.uint64)
        d_out = d.up(blank)
        cases = [
            (lambda: engine.fr_lincomb_device(0, n, [], [], d_out), "k = 0"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a] * 5, [1] * 5, d_out), "k = 5"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a, None], [1, 2], d_out), r"d_v\[1\]: null"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a], [1], None), "d_out: null"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a, at(d_b, 4)], [1, 2], d_out), "not aligned"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a, d_b], [1, 2], at(d_b, rec)), r"d_v\[1\] and d_out overlap"),
            (lambda: engine.fr_lincomb_device(0, n, [at(d_a, rec), d_b], [1, 2], d_a), r"d_v\[0\] and d_out overlap"),
            (lambda: engine.fr_lincomb_device(0, n, [d_a], np.frombuffer(f.r.to_bytes(rec, "little"), dtype="<u8").astype(np.uint64), d_out),
             r"scalars\[0\]: not below r"),
        ]
        for call, message in cases:
            with pytest.raises(libff_amd.AmdMsmError, match=message) as e:
                call()
            assert e.value.code == BAD_ARG, message
        with pytest.raises(libff_amd.AmdMsmError, match="2\\^28") as e:
            engine.fr_lincomb_device(0, (1 << 28) + 1, [d_a], [1], d_out)
        assert e.value.code == TOO_LARGE
        assert "n = " in err()
        engine.fr_lincomb_device(0, 0, [None, None], [1, 2], None)   # n = 0: nothing is looked at but the scalars
        assert (d.down(d_out, blank.shape) == SENTINEL).all() and (d.down(d_a, a.shape) == a).all()
        # a vector listed twice, written in place: 3 a - a = 2 a
        engine.fr_lincomb_device(0, n, [d_a, d_a], [3, f.r - 1], d_a)
        assert f.ints(d.down(d_a, (n, f.limbs)), False) == [2 * x % f.r for x in f.ints(a[:n], False)]


# ---- the generator's evaluation, from t to a key vector -----------------------------------------------------------------
@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4")])
def test_instance_map_with_evaluation(engine, curve):
    """40 constraints, 3 inputs, 60 variables (the constant 1 is variable 0), a domain of 48 points.  u = L(t) from the device; At, Bt, Ct from
    three transposed handles, A with the input-consistency rows; for a random assignment z, <At, z> = A_z(t) with A_z the
    inverse transform of M_A z evaluated by Horner's rule, the same for B and C; then (beta At + alpha Bt + Ct) / delta"""
    f = fm.field(curve)
    r, rec = f.r, f.limbs * 8
    n_con, n_in, n_var = 40, 3, 60
    m = libff_amd.fr_domain(curve, n_con + n_in + 1)["m"]
    assert m == 48   # 32 + 16: the step domain libfqfft chooses for 44
    rng = random.Random(curve)
    lengths = [1 + rng.randrange(6) for _ in range(n_con)]
    mats = [mm.random_matrix(r, lengths, n_var, seed=40 + i, nonzero=False) for i in range(3)]
    # row num_constraints + i of A is the variable i, i = 0 .. num_inputs: At[i] += u[num_constraints + i]
    mats[0] = mm.Csr(mats[0].rows + [[(i, 1)] for i in range(n_in + 1)], n_var)
    t = point(curve, m)
    z = [1] + mm.random_x(r, n_var - 1, seed=9)
    alpha, beta, delta = (rng.randrange(1, r) for _ in range(3))
    with Dev(engine) as d:
        d_u = d.buf(m * rec)
        engine.fr_domain_lagrange_device(curve, m, t, d_u)
        u = f.ints(d.down(d_u, (m, f.limbs)), False)
        assert u == lm.lagrange_def(curve, m, t)
        d_t, evals = [], []
        for mat in mats:
            with engine.fr_matrix_load_transposed(curve, *mat.arrays(f, False), n_var) as h:
                d_v = d.buf(n_var * rec)
                engine.fr_matrix_apply_device(h, d_u, m, d_v, n_var)
                got = f.ints(d.down(d_v, (n_var, f.limbs)), False)
            assert got == mm.apply(lm.transpose(mat), u, r)
            # the witness side of the same matrix: M z on the domain, interpolated, evaluated at t
            rows = mm.apply(mat, z, r, n_out=m)
            coeffs = f.ints(engine.fr_domain_fft(curve, f.records(rows, False), inverse=True), False)
            assert sum(x * y for x, y in zip(got, z)) % r == poly_eval(coeffs, t, r)
            d_t.append(d_v)
            evals.append(got)
        di = pow(delta, -1, r)
        d_key = d.buf(n_var * rec)
        engine.fr_lincomb_device(curve, n_var, d_t, [beta * di, alpha * di, di], d_key)
        want = [(beta * a + alpha * b + c) * di % r for a, b, c in zip(*evals)]
        assert f.ints(d.down(d_key, (n_var, f.limbs)), False) == want
