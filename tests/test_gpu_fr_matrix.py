"""Sparse matrix times Fr vector on the device (Engine.fr_matrix_load / fr_matrix_apply / fr_matrix_apply_device), all
six scalar fields, the default path and the straightforward one behind AMDMSM_FR_MATRIX_NAIVE=1.  Expected values come
from tests/fr_matrix_model.py -- Python integers, the definition -- and everything is compared bit for bit, as
records.  Nothing here knows how a matrix is stored: the row lengths are chosen from what libff_amd.plan_fr_matrix
reports (the thresholds between the row classes, the chain length T of the field)."""
import ctypes
import random

import numpy as np
import pytest

import fr_matrix_model as model
import group_fft_model as gmodel
from fr_dev import BAD_ARG, FOUR, OK, SENTINEL, TOO_LARGE, UNSUPPORTED, Dev, at, env_path, hip_runtime, poly_eval
from fr_fft_model import GENERATOR
from fr_fft_model import fft as model_fft

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, multi_exp_base_form_special, plan_fr_matrix  # noqa: E402

CURVES = sorted(model.CURVES)
IDS = [model.CURVES[c] for c in CURVES]
PATHS = [pytest.param(False, id="resident"), pytest.param(True, id="naive")]


def path(naive):
    """the environment of a load: AMDMSM_FR_MATRIX_NAIVE decides the form the handle keeps"""
    return env_path("AMDMSM_FR_MATRIX_NAIVE", naive)


def load(engine, curve, m, plain, naive):
    f = model.field(curve)
    with path(naive):
        return engine.fr_matrix_load(curve, *m.arrays(f, plain), m.n_cols, plain=plain)


def thresholds(curve):
    f = model.field(curve)
    p = plan_fr_matrix(curve, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros((0, f.limbs), dtype=np.uint64), 0)
    return p["wave_row"], p["split_row"], p["chunk"]


_cases = {}


def big_case(curve):
    """about 300 rows by 200 columns with every row length at which the library changes its path; computed once"""
    if curve not in _cases:
        f = model.field(curve)
        t1, t2, _ = thresholds(curve)
        lens = [0, 1, 2, 3]
        for t in (t1, t2):
            lens += [t - 1, t, t + 1]
        if t2 > 1 << 16:
            lens[-1] = (1 << 16) + 1
        rng = random.Random(curve)
        lens += [rng.choice((0, 1, 1, 2, 2, 3, 4, 8, 9, t1 + 5)) for _ in range(300 - len(lens))]
        rng.shuffle(lens)
        m = model.random_matrix(f.r, lens, 200, seed=7 + curve)
        # zeros too, in rows of their own so that the lengths above stay what they are
        m = model.Csr(m.rows + model.random_matrix(f.r, [5, 40, t1 + 3], 200, seed=curve, nonzero=False).rows, 200)
        x = model.random_x(f.r, 200, seed=70 + curve)
        _cases[curve] = (m, x, model.apply(m, x, f.r))
    return _cases[curve]


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_all_fields_both_forms(engine, curve, naive):
    f = model.field(curve)
    m, x, want = big_case(curve)
    p = plan_fr_matrix(curve, *m.arrays(f, True), m.n_cols, plain=True)
    assert p["rows_split"] >= 1 and p["rows_wave"] >= 3 and p["rows_lane"] >= 200
    for plain in (False, True):
        with load(engine, curve, m, plain, naive) as mat:
            got = engine.fr_matrix_apply(mat, f.records(x, plain), plain=plain)
            assert got.shape == (m.n_rows, f.limbs)
            assert (got == f.records(want, plain)).all(), plain
    # the coefficients in one form, the vector in the other: the forms are independent
    with load(engine, curve, m, True, naive) as mat:
        assert (engine.fr_matrix_apply(mat, f.records(x, False)) == f.records(want, False)).all()


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_worst_cases_of_the_accumulators(engine, curve, naive):
    f = model.field(curve)
    r = f.r
    t1, t2, T = thresholds(curve)
    assert T == model.chunk_rule(r, f.words)
    n_cols = 16
    rng = random.Random(curve)
    col = lambda: rng.randrange(n_cols)
    rows = [[(col(), r - 2) for _ in range(n)] for n in (T, T + 1, 3 * T + 1)]
    if 64 * (T + 1) + 1 <= 20000:   # a chain of T and of T + 1 in every lane of a wave
        rows += [[(col(), r - 2) for _ in range(n)] for n in (64 * T, 64 * (T + 1) + 1)]
    rows += [[(col(), 1) for _ in range(70000)], [(col(), r - 1) for _ in range(70000)]]
    cancel = [(c % n_cols, v) for c in range(150) for v in (rng.randrange(2, r - 1),)]
    rows += [[(0, 1), (0, r - 1), (1, 5), (1, r - 5)], cancel + [(c, r - v) for c, v in cancel]]
    rows += [[(col(), r - 2) for _ in range(T + 1)] + [(col(), 1)] * 3 + [(col(), r - 1)] * 2]
    m = model.Csr(rows, n_cols)
    x = [r - 1] * n_cols
    want = model.apply(m, x, r)
    assert want[-3] == 0 and want[-2] == 0
    for plain in (False, True):
        with load(engine, curve, m, plain, naive) as mat:
            got = engine.fr_matrix_apply(mat, f.records(x, plain), plain=plain)
            assert (got == f.records(want, plain)).all(), plain


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(5, id="mnt6")])
def test_shapes(engine, curve, naive):
    f = model.field(curve)
    r = f.r
    none = np.zeros((0, f.limbs), dtype=np.uint64)
    # no rows: nothing is written, or only zeros
    with load(engine, curve, model.Csr([], 0), False, naive) as mat:
        assert engine.fr_matrix_apply(mat, none).shape == (0, f.limbs)
        assert (engine.fr_matrix_apply(mat, none, n_out=5) == 0).all()
    # rows without entries
    with load(engine, curve, model.Csr([[], [], []], 4), False, naive) as mat:
        assert (engine.fr_matrix_apply(mat, f.records([1, 2, 3, 4], False), n_out=4) == 0).all()
    # one row, duplicate and unsorted columns, a longer vector than the matrix has columns
    one = model.Csr([[(3, 2), (0, r - 1), (3, 5), (1, 1), (3, r - 7)]], 4)
    x = model.random_x(r, 9, seed=curve)
    with load(engine, curve, one, True, naive) as mat:
        got = engine.fr_matrix_apply(mat, f.records(x, True), plain=True)
        assert f.ints(got, True) == [(-x[0] + x[1]) % r]
    # one below, at and above a workgroup's worth of rows, and of a wave's
    for n_rows in (63, 64, 65, 255, 256, 257):
        rng = random.Random(n_rows)
        m = model.random_matrix(r, [rng.randrange(5) for _ in range(n_rows)], 33, seed=n_rows, nonzero=False)
        x = model.random_x(r, 40, seed=n_rows + 1)
        with load(engine, curve, m, False, naive) as mat:
            got = engine.fr_matrix_apply(mat, f.records(x, False))
            assert (got == f.records(model.apply(m, x, r), False)).all(), n_rows


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR[:3])
def test_zero_tail_and_device_entry(engine, curve, naive):
    """the device entry on garbage: the rows, zeros up to n_out, and nothing at or beyond n_out"""
    f = model.field(curve)
    rec = f.limbs * 8
    t1, t2, _ = thresholds(curve)
    m = model.random_matrix(f.r, [3, 0, 1, t1 + 1, 2, t2 + 1, 5, 0, 0, 1, 2], 50, seed=3 * curve)
    x = model.random_x(f.r, 50, seed=5)
    hip = hip_runtime()
    with load(engine, curve, m, False, naive) as mat, Dev(engine) as d:
        d_x = d.up(f.records(x, False))
        for n_out in (m.n_rows, m.n_rows + 1, 16, 64, 200):
            want = f.records(model.apply(m, x, f.r, n_out), False)
            d_out = d.up(np.full((n_out + 3, f.limbs), SENTINEL, dtype=np.uint64))
            engine.fr_matrix_apply_device(mat, d_x, 50, at(d_out, 2 * rec), n_out)
            got = d.down(d_out, (n_out + 3, f.limbs))
            assert (got[2:-1] == want).all(), n_out
            assert (got[:2] == SENTINEL).all() and (got[-1] == SENTINEL).all(), n_out
        # on a stream of the caller's
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        try:
            d_out = d.up(np.full((16, f.limbs), SENTINEL, dtype=np.uint64))
            engine.fr_matrix_apply_device(mat, d_x, 50, d_out, 16, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
        finally:
            assert hip.hipStreamDestroy(stream) == 0
        assert (d.down(d_out, (16, f.limbs)) == f.records(model.apply(m, x, f.r, 16), False)).all()


@pytest.mark.parametrize("naive", PATHS)
def test_two_streams_two_handles(engine, naive):
    curve = 1
    f = model.field(curve)
    _, t2, _ = thresholds(curve)
    ma = model.random_matrix(f.r, [2, 70, 3 * t2 + 5, 1, 0, 9], 40, seed=1)
    mb = model.random_matrix(f.r, [1, 1, 4, 2 * t2 + 1, 33], 40, seed=2)
    xs = [model.random_x(f.r, 40, seed=s) for s in (11, 12)]
    hip = hip_runtime()
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        with Dev(engine) as d:
            a, b = load(engine, curve, ma, False, naive), load(engine, curve, mb, True, naive)
            d_x = [d.up(f.records(x, False)) for x in xs]
            outs = [d.up(np.full((8, f.limbs), SENTINEL, dtype=np.uint64)) for _ in range(4)]
            # one handle on two streams, the other handle between them
            engine.fr_matrix_apply_device(a, d_x[0], 40, outs[0], 8, stream=streams[0])
            engine.fr_matrix_apply_device(a, d_x[1], 40, outs[1], 8, stream=streams[1])
            engine.fr_matrix_apply_device(b, d_x[0], 40, outs[2], 8, stream=streams[1])
            engine.fr_matrix_apply_device(b, d_x[1], 40, outs[3], 8, stream=streams[0])
            a.free()   # waits for both streams' use of it
            for s in streams:
                assert hip.hipStreamSynchronize(s) == 0
            b.free()
            for out, (m, x) in zip(outs, ((ma, xs[0]), (ma, xs[1]), (mb, xs[0]), (mb, xs[1]))):
                assert (d.down(out, (8, f.limbs)) == f.records(model.apply(m, x, f.r, 8), False)).all()
            # freed handles are refused, by both entries, and so is freeing one twice
            with pytest.raises(libff_amd.AmdMsmError, match="handle"):
                engine.fr_matrix_apply_device(libff_amd.FrMatrix(engine, 1 << 40, curve, 6, 40), d_x[0], 40, outs[0], 8)
            assert engine.lib.amdmsm_fr_matrix_free(engine.h, ctypes.c_uint64(1 << 40)) == BAD_ARG
    finally:
        for s in streams:
            assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_refused_loads_name_the_entry(engine, curve):
    f = model.field(curve)
    r = f.r
    m = model.Csr([[(2, 1), (0, 7)], [], [(4, r - 1), (1, 3), (3, 9)]], 5)
    off, cols, co = m.arrays(f, True)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: engine.lib.amdmsm_last_error(engine.h)

    def call(c, n_rows, n_cols, o, cc, v, plain=True):
        h = ctypes.c_uint64(99)
        rc = engine.lib.amdmsm_fr_matrix_load(engine.h, c, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(o), ptr(cc), ptr(v),
                                              int(plain), ctypes.byref(h))
        if rc != OK:
            assert h.value == 0
        return rc, h.value

    assert call(6, 3, 5, off, cols, co)[0] == UNSUPPORTED
    bad = off.copy()
    bad[0] = 1
    assert call(curve, 3, 5, bad, cols, co)[0] == BAD_ARG and b"offsets[0]" in err()
    bad = off.copy()
    bad[2] = 1
    assert call(curve, 3, 5, bad, cols, co)[0] == BAD_ARG and b"row 1" in err()
    assert call(curve, 3, 4, off, cols, co)[0] == BAD_ARG and b"entry 2" in err() and b"column 4" in err()
    for plain in (False, True):
        big = m.arrays(f, plain)[2].copy()
        big[3] = np.frombuffer(r.to_bytes(8 * f.limbs, "little"), dtype="<u8")
        assert call(curve, 3, 5, off, cols, big, plain)[0] == BAD_ARG and b"entry 3" in err() and b">= r" in err()
    assert call(curve, 3, 5, None, cols, co)[0] == BAD_ARG and b"offsets" in err()
    assert call(curve, 3, 5, off, None, co)[0] == BAD_ARG and b"cols" in err()
    assert call(curve, 3, 5, off, cols, None)[0] == BAD_ARG and b"coeffs" in err()
    assert call(curve, (1 << 28) + 1, 5, off, cols, co)[0] == TOO_LARGE and b"2^28" in err()
    assert call(curve, 3, (1 << 28) + 1, off, cols, co)[0] == TOO_LARGE and b"2^28" in err()
    huge = np.array([0, 0, 0, (1 << 31) + 1], dtype=np.uint64)
    assert call(curve, 3, 5, huge, cols, co)[0] == TOO_LARGE and b"2^31" in err()
    assert engine.lib.amdmsm_fr_matrix_load(engine.h, curve, ctypes.c_size_t(3), ctypes.c_size_t(5), ptr(off), ptr(cols), ptr(co), 1,
                                            None) == BAD_ARG
    rc, h = call(curve, 3, 5, off, cols, co)   # and with every rule kept the same call loads
    assert rc == OK and h != 0
    assert engine.lib.amdmsm_fr_matrix_free(engine.h, ctypes.c_uint64(h)) == OK


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR[:3])
def test_refused_applies_leave_the_output_alone(engine, curve, naive):
    """both apply entries, with a context: the code, what amdmsm_last_error names, the output untouched"""
    f = model.field(curve)
    rec = f.limbs * 8
    m = model.random_matrix(f.r, [2, 0, 5, 1], 6, seed=curve)
    x = model.random_x(f.r, 6, seed=1)
    recs = f.records(x, False)
    want = f.records(model.apply(m, x, f.r, 8), False)
    o, bad_opts = engine._opts(), engine._opts()
    bad_opts.struct_size += 8
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: engine.lib.amdmsm_last_error(engine.h)
    other = libff_amd.Engine(0)
    try:
        mat, foreign = load(engine, curve, m, False, naive), load(other, curve, m, False, naive)
        gone = load(engine, curve, m, False, naive)
        gone_id = gone.handle
        gone.free()

        def cases(call, src, dst, read):
            def refused(code, word, *args):
                assert call(*args) == code and word in err(), (word, err())
                assert (read() == SENTINEL).all(), word

            refused(BAD_ARG, b"handle", foreign.handle, src, 6, dst, 8, o)
            refused(BAD_ARG, b"handle", gone_id, src, 6, dst, 8, o)
            refused(BAD_ARG, b"handle", 0, src, 6, dst, 8, o)
            refused(BAD_ARG, b"n_x", mat.handle, src, 5, dst, 8, o)
            refused(BAD_ARG, b"n_out", mat.handle, src, 6, dst, 3, o)
            refused(BAD_ARG, b"x: null", mat.handle, None, 6, dst, 8, o)
            refused(BAD_ARG, b"output", mat.handle, src, 6, None, 8, o)
            refused(BAD_ARG, b"struct_size", mat.handle, src, 6, dst, 8, bad_opts)
            refused(TOO_LARGE, b"2^28", mat.handle, src, 6, dst, (1 << 28) + 1, o)
            assert call(mat.handle, src, 6, dst, 8, o) == OK

        def host(h, src, n_x, dst, n_out, opts):
            return engine.lib.amdmsm_fr_matrix_apply(engine.h, ctypes.c_uint64(h), src, ctypes.c_size_t(n_x), dst, ctypes.c_size_t(n_out),
                                                     ctypes.byref(opts))

        def dev(h, src, n_x, dst, n_out, opts):
            return engine.lib.amdmsm_fr_matrix_apply_device(engine.h, ctypes.c_uint64(h), src, ctypes.c_size_t(n_x), dst,
                                                            ctypes.c_size_t(n_out), ctypes.byref(opts))

        out = np.full((8, f.limbs), SENTINEL, dtype=np.uint64)
        cases(host, ptr(recs), ptr(out), lambda: out)
        assert (out == want).all()
        with Dev(engine) as d:
            d_x, d_out = d.up(recs), d.up(np.full((8, f.limbs), SENTINEL, dtype=np.uint64))
            read = lambda: d.down(d_out, (8, f.limbs))
            cases(dev, d_x, d_out, read)
            assert (read() == want).all()
            # the device entry's own rules: alignment, and an output that overlaps the vector
            d_big = d.up(np.full((16, f.limbs), SENTINEL, dtype=np.uint64))
            engine.h2d(d_big, recs)
            big = lambda: d.down(d_big, (16, f.limbs))
            before = big()
            assert dev(mat.handle, d_x, 6, at(d_big, 4), 8, o) == BAD_ARG and b"aligned" in err()
            assert dev(mat.handle, at(d_big, 4), 6, d_out, 8, o) == BAD_ARG and b"aligned" in err()
            assert dev(mat.handle, d_big, 6, at(d_big, 5 * rec), 8, o) == BAD_ARG and b"overlap" in err()
            assert dev(mat.handle, at(d_big, 7 * rec), 6, d_big, 8, o) == BAD_ARG and b"overlap" in err()
            assert dev(mat.handle, d_big, 6, d_big, 8, o) == BAD_ARG and b"overlap" in err()
            assert (big() == before).all()
            assert dev(mat.handle, d_big, 6, at(d_big, 6 * rec), 8, o) == OK   # next to each other is not overlapping
            assert (big()[6:14] == want).all() and (big()[14:] == SENTINEL).all()
        mat.free()
        foreign.free()
    finally:
        other.close()


def test_a_record_that_is_no_field_element_stays_in_its_rows(engine):
    """x[c] >= r: unspecified values in the rows that read column c, every other row and the tail as they should be"""
    curve = 3
    f = model.field(curve)
    t1, t2, _ = thresholds(curve)
    m = model.random_matrix(f.r, [3, t1 + 2, 0, 2, t2 + 3, 1, 4], 30, seed=4)
    x = model.random_x(f.r, 30, seed=6)
    recs = f.records(x, False)
    recs[7] = np.uint64(0xffffffffffffffff)
    want = f.records(model.apply(m, x, f.r, 16), False)
    clean = [i for i, row in enumerate(m.rows) if all(c != 7 for c, _ in row)] + list(range(m.n_rows, 16))
    assert len(clean) > 9
    with load(engine, curve, m, False, False) as mat:
        got = engine.fr_matrix_apply(mat, recs, n_out=16)
    assert (got[clean] == want[clean]).all()


@pytest.mark.parametrize("naive", PATHS)
def test_from_the_assignment_to_the_quotient(engine, port, naive):
    """a satisfied constraint system -- z_{k+2} = z_k z_{k+1} and a few linear rows -- from z on the device to Az o Bz - Cz
    = 0, to the h of the seven-transform recipe, and to an MSM over the apply's output"""
    curve, n = 0, 64
    f = model.field(curve)
    r, g, w = f.r, GENERATOR[curve], f.root(n)
    rng = random.Random(5)
    z = [1, rng.randrange(r), rng.randrange(r)]
    A, B, C = [], [], []
    for k in range(1, 41):   # z_{k+2} = z_k * z_{k+1}
        z.append(z[k] * z[k + 1] % r)
        A.append([(k, 1)])
        B.append([(k + 1, 1)])
        C.append([(k + 2, 1)])
    for k in range(10):   # (sum of a few terms) * 1 = a new variable
        terms = [(rng.randrange(len(z)), rng.choice((1, r - 1, 2, rng.randrange(r)))) for _ in range(3 + 20 * (k % 2))]
        z.append(sum(v * z[c] for c, v in terms) % r)
        A.append(terms)
        B.append([(0, 1)])
        C.append([(len(z) - 1, 1)])
    n_cols = len(z)
    mats = [model.Csr(rows, n_cols) for rows in (A, B, C)]
    az, bz, cz = (model.apply(m, z, r, n) for m in mats)
    assert all((a * b - c) % r == 0 for a, b, c in zip(az, bz, cz)) and len(A) < n
    k_inv = pow(pow(g, n, r) - 1, -1, r)
    gname = "alt_bn128_g1"
    grp = gmodel.group_of(port, gname)
    logs = [random.Random(9).randrange(1, grp.r) for _ in range(n)]
    s = libff_amd.sizes(grp.curve, grp.group)
    with Dev(engine) as d:
        handles = [load(engine, curve, m, True, naive) for m in mats]
        d_z = d.up(f.records(z, False))
        bufs = [d.up(np.full((n, f.limbs), SENTINEL, dtype=np.uint64)) for _ in range(3)]
        for h, p in zip(handles, bufs):
            engine.fr_matrix_apply_device(h, d_z, n_cols, p, n)
        got = [f.ints(d.down(p, (n, f.limbs)), False) for p in bufs]
        assert got == [az, bz, cz]
        d_h = d.buf(n * f.limbs * 8)
        engine.fr_muladd_device(curve, n, bufs[0], bufs[1], d_h, d_c=bufs[2])
        assert (d.down(d_h, (n, f.limbs)) == 0).all()
        # the apply's output as the scalars of an MSM, without a host copy
        d_xyz, d_aff, d_pt = d.up(grp.records(logs)), d.buf(n * s["affine_bytes"]), d.buf(s["g_bytes"])
        engine.import_bases_device(grp.curve, grp.group, d_xyz, s["g_bytes"], multi_exp_base_form_special, n, d_aff)
        engine.msm_device(grp.curve, grp.group, d_aff, bufs[0], n, d_pt, out_form=OUT_AFFINE)
        assert (d.down(d_pt, (1, grp.gl)) == grp.records([sum(x * y for x, y in zip(az, logs)) % grp.r])).all()
        # the quotient: three inverse transforms, three coset transforms, the product step, one inverse coset transform
        for p in bufs:
            engine.fr_fft_device(curve, p, n, p, inverse=True)
            engine.fr_fft_device(curve, p, n, p, coset=g)
        engine.fr_muladd_device(curve, n, bufs[0], bufs[1], d_h, d_c=bufs[2], k=k_inv)
        engine.fr_fft_device(curve, d_h, n, d_h, coset=g, inverse=True)
        h = f.ints(d.down(d_h, (n, f.limbs)), False)
        for m in handles:
            m.free()
    winv, ninv = pow(w, -1, r), pow(n, -1, r)
    pa, pb, pc = (model_fft(v, winv, r, scale=ninv) for v in (az, bz, cz))
    tau = rng.randrange(r)
    lhs = (poly_eval(pa, tau, r) * poly_eval(pb, tau, r) - poly_eval(pc, tau, r)) % r
    assert lhs == poly_eval(h, tau, r) * (pow(tau, n, r) - 1) % r
    assert any(h)
