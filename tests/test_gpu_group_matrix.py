"""Sparse matrix times point vector on the handle of an Fr matrix (Engine.group_matrix_apply / _device /
plan_group_matrix), all eleven groups.  Expected values come from tests/group_matrix_model.py: every input point is a
known multiple of the generator, every expected row the generator times the row of fr_matrix_model.apply over those
multiples.  Records are compared bit for bit in special form.  Nothing here knows how the handle stores its entries.

The small matrices are loaded with AMDMSM_FR_MATRIX_WAVE_ROW=4 and AMDMSM_FR_MATRIX_SPLIT_ROW=64, so that 24 points and
about 80 rows reach every kind of wave job.  bw6_761 keeps at most 40 general entries: a ladder of its 24-word field
takes about 45 ms whatever the count."""
import ctypes
import random

import numpy as np
import pytest

import fr_matrix_model as mm
import group_matrix_model as model
from fr_dev import BAD_ARG, OK, SENTINEL, TOO_LARGE, UNSUPPORTED, Dev, env_path, hip_runtime

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G2, MNT6, OUT_AFFINE, OUT_LIBFF, fft_twiddles, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special)

ALL = [pytest.param(n, id=n) for n in model.ALL_NAMES]
SPECIAL, NORMAL = multi_exp_base_form_special, multi_exp_base_form_normal
FORMS = (OUT_LIBFF, OUT_AFFINE)


def host(engine, g, mat, pts, out_form=OUT_AFFINE, base_form=SPECIAL, **kw):
    """the host entry, result in special form whatever the output form"""
    got = engine.group_matrix_apply(mat, g.group, pts, base_form=base_form, out_form=out_form, **kw)
    return model.special(g, got, out_form)


def device(engine, d, g, mat, pts, guard=2, out_form=OUT_AFFINE, **kw):
    """the device entry on special-form records; returns (the buffer of the output, rows + guard sentinel records)"""
    s = libff_amd.sizes(g.curve, g.group)
    n = len(pts)
    d_aff = d.buf(n * s["affine_bytes"])
    if n:
        engine.import_bases_device(g.curve, g.group, d.up(pts), s["g_bytes"], SPECIAL, n, d_aff)
        engine.synchronize()   # the import ran on the context's stream, the apply may run on another
    d_out = d.up(np.full((mat.n_rows + guard, g.gl), SENTINEL, dtype=np.uint64))
    engine.group_matrix_apply_device(mat, g.group, d_aff, n, d_out, out_form=out_form, **kw)
    return d_out, mat.n_rows + guard


def rows_and_guard(d, g, mat, d_out, total, out_form):
    got = d.down(d_out, (total, g.gl))
    return model.special(g, got[:mat.n_rows], out_form), got[mat.n_rows:]


@pytest.mark.parametrize("name", ALL)
def test_every_job_kind(engine, port, name):
    g, m, logs, pts, want = model.small_case(port, name)
    f = model.field_of(g)
    with model.env(model.SMALL):
        fr_plan = libff_amd.plan_fr_matrix(g.curve, *m.arrays(f, True), m.n_cols, plain=True)
    counts = mm.class_counts(m, g.r)
    with model.load(engine, g, m) as mat:
        plan = engine.plan_group_matrix(mat, g.group)
        assert plan["general"] == counts["general"] > 0
        assert plan["plus_minus_one"] == counts["plus_one"] + counts["minus_one"] > 0
        assert fr_plan["rows_split"] == 3 and plan["partials"] == fr_plan["partials"] == 2 + 2 + 3
        assert fr_plan["rows_lane"] > 64 and fr_plan["rows_wave"] == 4 and plan["wave_jobs"] == fr_plan["wave_jobs"]
        assert plan["chunks"] == 1 and plan["workspace_bytes"] > 0 and plan["launches"] == 5 + 1
        if name.startswith("bw6_761"):
            assert plan["general"] <= 40
        for out_form in FORMS:
            assert (host(engine, g, mat, pts, out_form) == want).all(), out_form
        normal = g.scale(pts, seed=7)
        assert (normal != pts).any()
        assert (host(engine, g, mat, normal, OUT_AFFINE, NORMAL) == want).all()
        with Dev(engine) as d:
            for out_form in FORMS:
                d_out, total = device(engine, d, g, mat, pts, out_form=out_form)
                got, guard = rows_and_guard(d, g, mat, d_out, total, out_form)
                assert (got == want).all(), out_form
                assert (guard == SENTINEL).all()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_381_g2"])
def test_default_thresholds(engine, port, name):
    """rows of 31, 32, 1024 and 1025 entries of +-1 over 16 points: a lane, one wave, one wave of 16 steps, two pieces"""
    g = model.gm.group_of(port, name)
    rng = random.Random(3)
    rows = [[(rng.randrange(16), rng.choice((1, g.r - 1))) for _ in range(n)] for n in (31, 32, 1024, 1025)]
    m = mm.Csr(rows, 16)
    logs = [rng.randrange(1, g.r) for _ in range(16)]
    pts, want = g.records(logs), model.expected(g, m, logs)
    with model.load(engine, g, m, small=False) as mat:
        plan = engine.plan_group_matrix(mat, g.group)
        assert plan["general"] == 0 and plan["plus_minus_one"] == m.nnz and plan["partials"] == 2 and plan["wave_jobs"] == 5
        assert plan["launches"] == 2
        for out_form in FORMS:
            assert (host(engine, g, mat, pts, out_form) == want).all(), out_form


@pytest.mark.parametrize("name", ["alt_bn128_g1", "mnt4_g2", "bw6_761_g1"])
def test_coefficient_classes_alone(engine, port, name):
    g, m0, logs, pts, _ = model.small_case(port, name)
    rng = random.Random(9)
    general = lambda: (2, g.r - 2, pow(2, rng.randrange(2, g.r.bit_length() + 40), g.r), rng.randrange(2, g.r - 1))[rng.randrange(4)]
    budget = [40 if name.startswith("bw6_761") else 1 << 30]

    def gen_or_one():   # bw6_761: all the general entries the time allows, the rest of the shape +1
        budget[0] -= 1
        return general() if budget[0] >= 0 else 1

    for label, pick in (("plus", lambda: 1), ("minus", lambda: g.r - 1), ("general", gen_or_one)):
        m = mm.Csr([[(c, pick()) for c, _ in row] for row in m0.rows], m0.n_cols)
        counts = mm.class_counts(m, g.r)
        with model.load(engine, g, m) as mat:
            plan = engine.plan_group_matrix(mat, g.group)
            assert (plan["general"], plan["plus_minus_one"]) == (counts["general"], counts["plus_one"] + counts["minus_one"])
            if label != "general":
                assert plan["general"] == 0
            elif not name.startswith("bw6_761"):
                assert plan["plus_minus_one"] == 0
            assert (host(engine, g, mat, pts) == model.expected(g, m, logs)).all(), label


@pytest.mark.parametrize("name", ALL)
def test_degenerate_additions(engine, port, name):
    """equal points, opposite points and infinity in the lane additions, at every round of the wave fold and in the
    combine.  Under the small thresholds the rows of 64 entries take one wave and those of 128 are split; under the
    default ones every row of up to 4 entries is a lane's, and the rows of 64 and 128 take one wave."""
    g = model.gm.group_of(port, name)
    m, logs = model.degenerate_matrix(g), model.degenerate_logs(g)
    pts, want = g.records(logs), model.expected(g, m, logs)
    z = 2 * (g.gl // 3)
    assert not any(want[i][z:].any() for i in (1, 2, 3, 9, 11)) and all(want[i][z:].any() for i in (0, 4, 5, 6, 8, 10))   # infinity
    for small in (True, False):
        with model.load(engine, g, m, small=small) as mat:
            plan = engine.plan_group_matrix(mat, g.group)
            assert plan["general"] == 3 and plan["partials"] == (4 if small else 0)
            for out_form in FORMS:
                assert (host(engine, g, mat, pts, out_form) == want).all(), (small, out_form)


@pytest.mark.parametrize("name", ["alt_bn128_g2", "mnt6_g1"])
def test_transposed_handle(engine, port, name):
    g, m, _, _, _ = model.small_case(port, name)
    rng = random.Random(21)
    logs = [rng.randrange(g.r) for _ in range(m.n_rows)]
    pts = g.records(logs)
    want = model.expected(g, model.transpose(m), logs)
    with model.load(engine, g, m, transposed=True) as mat:
        assert (mat.n_rows, mat.n_cols) == (m.n_cols, m.n_rows)
        assert (host(engine, g, mat, pts) == want).all()


def test_one_handle_two_worlds(engine, port):
    g1, m, logs, pts1, want1 = model.small_case(port, "bls12_381_g1")
    g2 = model.gm.group_of(port, "bls12_381_g2")
    f = model.field_of(g1)
    x = f.records(logs, False)
    want_fr = f.records(mm.apply(m, logs, g1.r), False)
    with model.load(engine, g1, m) as mat:
        first = engine.fr_matrix_apply(mat, x)
        assert (host(engine, g1, mat, pts1) == want1).all()
        assert (host(engine, g2, mat, g2.records(logs)) == model.expected(g2, m, logs)).all()
        second = engine.fr_matrix_apply(mat, x)
    assert (first == want_fr).all() and (second == first).all()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_381_g2", "mnt4_g1"])
def test_chunks(engine, port, name):
    g, m, logs, pts, want = model.small_case(port, name)
    with model.load(engine, g, m) as mat:
        assert engine.plan_group_matrix(mat, g.group, 16)["chunks"] >= 3
        assert engine.plan_group_matrix(mat, g.group, 1)["chunks"] >= engine.plan_group_matrix(mat, g.group, 16)["chunks"]
        raw = [engine.group_matrix_apply(mat, g.group, pts, base_form=SPECIAL, chunk_entries=c) for c in (0, 1, 16)]
        assert (raw[0] == raw[1]).all() and (raw[0] == raw[2]).all()   # the libff records themselves, bit for bit
        assert (g.special(raw[0]) == want).all()
        with Dev(engine) as d:
            d_out, total = device(engine, d, g, mat, pts, out_form=OUT_AFFINE, chunk_entries=16)
            got, guard = rows_and_guard(d, g, mat, d_out, total, OUT_AFFINE)
            assert (got == want).all() and (guard == SENTINEL).all()


def test_device_entry_streams_and_free(engine, port):
    g, m, logs, pts, want = model.small_case(port, "alt_bn128_g1")
    hip = hip_runtime()
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        with Dev(engine) as d:
            mat = model.load(engine, g, m)
            # one handle on two streams of the caller's
            outs = [device(engine, d, g, mat, pts, guard=3, out_form=form, stream=s) for form, s in zip(FORMS, streams)]
            # freed straight behind an apply nobody has waited for: the free waits
            last = device(engine, d, g, mat, pts, guard=3, out_form=OUT_AFFINE, stream=streams[0])
            mat.free()
            for s in streams:
                assert hip.hipStreamSynchronize(s) == 0
            for (d_out, total), form in zip(outs + [last], FORMS + (OUT_AFFINE,)):
                got, guard = rows_and_guard(d, g, mat, d_out, total, form)
                assert (got == want).all(), form
                assert guard.shape[0] == 3 and (guard == SENTINEL).all()
    finally:
        for s in streams:
            assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bw6_761_g2", "mnt4_g2"])
def test_empty_shapes(engine, port, name):
    g = model.gm.group_of(port, name)
    pts = g.records([3, 4, 5])
    zero = g.records([0])[0]
    z = ctypes.c_size_t(0)
    # no rows: nothing is written, null vectors will do
    with model.load(engine, g, mm.Csr([], 3)) as mat:
        assert engine.group_matrix_apply(mat, g.group, pts, base_form=SPECIAL).shape == (0, g.gl)
        o = engine._opts()
        assert engine.lib.amdmsm_group_matrix_apply_device(engine.h, g.curve, g.group, ctypes.c_uint64(mat.handle), None,
                                                           ctypes.c_size_t(3), None, z, ctypes.byref(o)) == OK
        assert engine.plan_group_matrix(mat, g.group)["wave_jobs"] == 0
    # rows without entries, and rows whose coefficients are all zero: the group's zero in both forms
    for m in (mm.Csr([[], [], []], 3), mm.Csr([[(0, 0)], [(1, 0), (2, 0)], [], [(0, 0)] * 70], 3)):
        with model.load(engine, g, m) as mat:
            plan = engine.plan_group_matrix(mat, g.group)
            assert plan["general"] == plan["plus_minus_one"] == plan["partials"] == 0
            for out_form in FORMS:
                got = engine.group_matrix_apply(mat, g.group, pts, base_form=SPECIAL, out_form=out_form)
                assert (got == zero).all(), out_form
                with Dev(engine) as d:
                    d_out, total = device(engine, d, g, mat, pts, out_form=out_form)
                    got = d.down(d_out, (total, g.gl))
                    assert (got[:m.n_rows] == zero).all() and (got[m.n_rows:] == SENTINEL).all()


def test_every_refusal(engine, port):
    g, m, logs, pts, want = model.small_case(port, "alt_bn128_g1")
    s = libff_amd.sizes(g.curve, g.group)
    lib, z = engine.lib, ctypes.c_size_t(0)
    n, n_rows = len(pts), m.n_rows
    other = libff_amd.Engine(0)
    with Dev(engine) as d:
        bufs = sorted((d.buf((n_rows + 2) * s["g_bytes"]), d.buf((n_rows + 2) * s["g_bytes"])), key=lambda p: p.value)
        d_out, d_aff = bufs   # the output below the points: no range of points reaches it
        engine.import_bases_device(g.curve, g.group, d.up(pts), s["g_bytes"], SPECIAL, n, d_aff)
        sentinel = np.full((n_rows + 2, g.gl), SENTINEL, dtype=np.uint64)
        engine.h2d(d_out, sentinel)
        hbuf = np.full((n_rows + 2 + n, g.gl), SENTINEL, dtype=np.uint64)   # host: the output, then the points
        hbuf[n_rows + 2:] = pts
        h_out, h_pts = hbuf[:n_rows + 2], hbuf[n_rows + 2:]
        mat = model.load(engine, g, m)
        freed = model.load(engine, g, m)
        freed_id = freed.handle
        freed.free()
        foreign = model.load(other, g, m)
        g381 = model.gm.group_of(port, "bls12_381_g1")
        other_curve = model.load(engine, g381, mm.Csr([[(0, 1)]], 1))
        with env_path("AMDMSM_FR_MATRIX_NAIVE", True):
            naive = model.load(engine, g, m, small=False)
        o, bad_o = engine._opts(), engine._opts()
        bad_o.struct_size += 4
        H = lambda h: ctypes.c_uint64(h)
        N = ctypes.c_size_t

        def dev(ctx=engine.h, curve=g.curve, group=g.group, h=mat.handle, p=d_aff, np_=n, out=d_out, opts=o):
            return lib.amdmsm_group_matrix_apply_device(ctx, curve, group, H(h), p, N(np_), out, z, ctypes.byref(opts))

        def hst(ctx=engine.h, curve=g.curve, group=g.group, h=mat.handle, p=h_pts.ctypes.data, stride=s["g_bytes"], np_=n,
                out=h_out.ctypes.data, opts=o):
            return lib.amdmsm_group_matrix_apply(ctx, curve, group, H(h), ctypes.c_void_p(p), N(stride), SPECIAL, N(np_),
                                                 ctypes.c_void_p(out), z, ctypes.byref(opts))

        def pln(ctx=engine.h, curve=g.curve, group=g.group, h=mat.handle, out=(ctypes.c_size_t * 8)()):
            return lib.amdmsm_plan_group_matrix(ctx, curve, group, H(h), z, out)

        def refused(code, word, *calls):
            for call in calls:
                assert call() == code, word
                if word:
                    msg = lib.amdmsm_last_error(engine.h if "ctx" not in word else None).decode()
                    assert word in msg, (word, msg)

        # 1. a group the library does not carry, before the context is looked at
        for ctx in (engine.h, None):
            refused(UNSUPPORTED, "", lambda: dev(ctx=ctx, curve=MNT6, group=G2), lambda: hst(ctx=ctx, curve=MNT6, group=G2),
                    lambda: pln(ctx=ctx, curve=MNT6, group=G2), lambda: dev(ctx=ctx, curve=9), lambda: hst(ctx=ctx, curve=9),
                    lambda: pln(ctx=ctx, curve=9), lambda: dev(ctx=ctx, group=3))
        # 2. bad arguments, each named
        refused(BAD_ARG, "ctx", lambda: dev(ctx=None), lambda: hst(ctx=None), lambda: pln(ctx=None))
        refused(BAD_ARG, "struct_size", lambda: dev(opts=bad_o), lambda: hst(opts=bad_o))
        for h in (freed_id, foreign.handle, 1 << 40):
            refused(BAD_ARG, "mat", lambda: dev(h=h), lambda: hst(h=h), lambda: pln(h=h))
        refused(BAD_ARG, "curve", lambda: dev(h=other_curve.handle), lambda: hst(h=other_curve.handle),
                lambda: pln(h=other_curve.handle))
        refused(BAD_ARG, "NAIVE", lambda: dev(h=naive.handle), lambda: hst(h=naive.handle), lambda: pln(h=naive.handle))
        refused(BAD_ARG, "n_points", lambda: dev(np_=n - 1), lambda: hst(np_=n - 1))
        refused(BAD_ARG, "d_points_affine", lambda: dev(p=None))
        refused(BAD_ARG, "points_xyz", lambda: hst(p=None))
        refused(BAD_ARG, "d_out_xyz", lambda: dev(out=None))
        refused(BAD_ARG, "out_xyz", lambda: hst(out=None))
        refused(BAD_ARG, "out", lambda: pln(out=None))
        refused(BAD_ARG, "stride", lambda: hst(stride=s["g_bytes"] - 8), lambda: hst(stride=s["g_bytes"] + 4))
        refused(BAD_ARG, "aligned", lambda: dev(p=ctypes.c_void_p(d_aff.value + 4)), lambda: dev(out=ctypes.c_void_p(d_out.value + 4)))
        refused(BAD_ARG, "overlap", lambda: dev(out=d_aff), lambda: dev(out=ctypes.c_void_p(d_aff.value + s["affine_bytes"])),
                lambda: hst(out=h_pts.ctypes.data), lambda: hst(out=h_pts.ctypes.data + 8 * s["g_bytes"]))
        # 3. too many points
        refused(TOO_LARGE, "n_points", lambda: dev(np_=(1 << 28) + 1), lambda: hst(np_=(1 << 28) + 1))
        # nothing was written, and the handle still serves
        engine.synchronize()
        assert (d.down(d_out, sentinel.shape) == SENTINEL).all() and (h_out == SENTINEL).all()
        assert dev() == OK and hst() == OK and pln() == OK
        assert (d.down(d_out, sentinel.shape)[:n_rows] != SENTINEL).all() and (d.down(d_out, sentinel.shape)[n_rows:] == SENTINEL).all()
        assert (g.special(h_out[:n_rows].copy()) == want).all() and (h_out[n_rows:] == SENTINEL).all()
        for h in (mat, other_curve, naive):
            h.free()
        foreign.free()
    other.close()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "alt_bn128_g2"])
def test_ceremony_route_against_trapdoor_route(engine, port, name):
    """[L_i(tau)]G from the powers [tau^i]G by the inverse group FFT and the fold by 1/n, then the transposed map; against
    L_i(tau) from the trapdoor, the same map over Fr on the same handle, and multiples of G by the model"""
    g = model.gm.group_of(port, name)
    f = model.field_of(g)
    n, tau = 8, 0x1d2c3b4a59687766554433221100ffeeddccbbaa
    rng = random.Random(8)
    rows = [[(rng.randrange(5), mm.pick_coeff(rng, g.r) or 1) for _ in range(rng.randrange(1, 4))] for _ in range(n)]
    m = mm.Csr(rows, 5)   # 8 constraints over 5 variables: the transposed handle has 5 rows and 8 columns
    powers = g.records([pow(tau, i, g.r) for i in range(n)])
    spectrum = engine.group_fft(g.curve, g.group, powers, fft_twiddles(g.curve, n, inverse=True), base_form=SPECIAL,
                                out_form=OUT_AFFINE, scalars_plain=True)
    lagrange = engine.fold_vec(g.curve, g.group, [spectrum], g.plain([pow(n, -1, g.r)]), base_form=SPECIAL, out_form=OUT_AFFINE,
                               scalars_plain=True)
    with model.load(engine, g, m, transposed=True) as mat:
        ceremony = host(engine, g, mat, lagrange)
        at = f.ints(engine.fr_matrix_apply(mat, engine.fr_domain_lagrange(g.curve, n, tau)), False)
    trapdoor = g.records(at)
    assert (ceremony == trapdoor).all()
    # and both are what the integers say
    lag = f.ints(engine.fr_domain_lagrange(g.curve, n, tau), False)
    assert at == mm.apply(model.transpose(m), lag, g.r)
