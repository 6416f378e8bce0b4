"""The R1CS-to-QAP witness map as one call (Engine.qap_witness_map / qap_witness_map_device) against the integer model
tests/qap_witness_model.py, coefficient by coefficient: a step and a basic domain, three fields, both record forms, with
and without blinding; bit for bit against the twelve single calls; the host entry, sentinels, refusals, phases, and h as
the scalars of an MSM."""
import random

import numpy as np
import pytest

import fr_fft_model as fm
import group_fft_model as gmodel
import qap_witness_model as qm
from fr_dev import BAD_ARG, SENTINEL, Dev, at

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, multi_exp_base_form_special  # noqa: E402

THREE = [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4"), pytest.param(2, id="bw6_761")]
N_COLS = 9
_expected = {}


def expected(curve, rows, m, blind):
    key = (curve, rows, m, blind)
    if key not in _expected:
        a, b, c, z = qm.random_system(curve, rows, N_COLS)
        _expected[key] = qm.witness_map(curve, a, b, c, z, m, blind)
    return _expected[key]


def blinding(curve):
    return tuple(fm.random_vector(curve, 3, seed=41))


def load(engine, curve, mats, plain):
    f = fm.field(curve)
    return [engine.fr_matrix_load(curve, *mt.arrays(f, plain), mt.n_cols, plain=plain) for mt in mats]


@pytest.mark.parametrize("curve", THREE)
@pytest.mark.parametrize("rows,m", [(43, 48), (60, 64)], ids=["step_32_16", "basic_64"])
def test_against_the_model(engine, curve, rows, m):
    f = fm.field(curve)
    assert libff_amd.fr_domain(curve, rows)["m"] == m
    assert libff_amd.plan_fr_qap_witness_map(curve, m)["kind"] == (libff_amd.DOMAIN_STEP_RADIX2 if m == 48 else libff_amd.DOMAIN_BASIC_RADIX2)
    a, b, c, z = qm.random_system(curve, rows, N_COLS)
    for plain in (False, True):
        mats = load(engine, curve, (a, b, c), plain)
        try:
            zr = f.records(z, plain)
            for blind in (None, blinding(curve)):
                want = expected(curve, rows, m, blind)
                h = engine.qap_witness_map(curve, *mats, zr, m, blind=blind, plain=plain)
                assert h.shape == (m + 1, f.limbs)
                assert f.ints(h, plain) == want, (curve, m, plain, blind is not None)
                if blind is None:
                    assert not h[m - 1].any() and not h[m].any()
                # the device entry: the same records, sentinels in front of d_h and behind d_h[m], z unchanged
                with Dev(engine) as d:
                    d_z = d.up(zr)
                    d_h = d.up(np.full((m + 5, f.limbs), SENTINEL, dtype=np.uint64))
                    engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, at(d_h, 2 * f.limbs * 8), blind=blind, plain=plain)
                    got = d.down(d_h, (m + 5, f.limbs))
                    assert (got[2:m + 3] == h).all(), (curve, m, plain)
                    assert (got[:2] == SENTINEL).all() and (got[m + 3:] == SENTINEL).all()
                    assert (d.down(d_z, zr.shape) == zr).all()
        finally:
            for mt in mats:
                mt.free()


def test_bit_for_bit_against_the_twelve_calls(engine):
    """m = 2^10 + 2^4 on alt_bn128: the sequence of test_gpu_fr_domain.py::test_quotient_on_a_step_domain, with the three
    applies in front, run here next to the one call"""
    curve, m = 0, (1 << 10) + (1 << 4)
    rows = m - 3
    f = fm.field(curve)
    rec = f.limbs * 8
    g = libff_amd.fr_multiplicative_generator(curve)
    a, b, c, z = qm.random_system(curve, rows, N_COLS, seed=3)
    zr = f.records(z, False)
    mats = load(engine, curve, (a, b, c), False)
    try:
        with Dev(engine) as d:
            d_z = d.up(zr)
            bufs = [d.buf(m * rec) for _ in range(3)]
            for mt, p in zip(mats, bufs):
                engine.fr_matrix_apply_device(mt, d_z, len(z), p, m)
            for p in bufs:
                engine.fr_domain_fft_device(curve, p, m, p, inverse=True)
                engine.fr_domain_fft_device(curve, p, m, p, coset=g)
            d_q = d.buf(m * rec)
            engine.fr_muladd_device(curve, m, bufs[0], bufs[1], d_q, d_c=bufs[2])
            engine.fr_domain_divide_by_z_device(curve, m, d_q, d_q, coset=g)
            engine.fr_domain_fft_device(curve, d_q, m, d_q, inverse=True, coset=g)
            twelve = d.down(d_q, (m, f.limbs))
            d_h = d.up(np.full((m + 2, f.limbs), SENTINEL, dtype=np.uint64))
            engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, d_h)
            got = d.down(d_h, (m + 2, f.limbs))
        assert (got[:m] == twelve).all() and (twelve != 0).any()
        assert not got[m - 1].any() and not got[m].any() and (got[m + 1] == SENTINEL).all()
        assert (engine.qap_witness_map(curve, *mats, zr, m) == got[:m + 1]).all()   # the host entry
    finally:
        for mt in mats:
            mt.free()


def test_refusals_and_the_context_afterwards(engine):
    curve, rows, m = 0, 43, 48
    f = fm.field(curve)
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    a, b, c, z = qm.random_system(curve, rows, N_COLS)
    zr = f.records(z, False)
    mats = load(engine, curve, (a, b, c), False)
    other = load(engine, 4, qm.random_system(4, rows, N_COLS)[:1], False)[0]
    tall = engine.fr_matrix_load(curve, *qm.random_system(curve, 60, N_COLS)[0].arrays(f, False), N_COLS)
    freed = load(engine, curve, (a,), False)[0]
    stale = libff_amd.FrMatrix(engine, freed.handle, curve, freed.n_rows, freed.n_cols)
    freed.free()
    try:
        with Dev(engine) as d:
            d_z = d.up(zr)
            d_h = d.up(np.full((m + 1, f.limbs), SENTINEL, dtype=np.uint64))
            run = lambda A=mats[0], B=mats[1], C=mats[2], n_z=len(z), mm=m, **kw: engine.qap_witness_map_device(curve, A, B, C, d_z, n_z, mm, d_h, **kw)
            cases = [
                (dict(B=other), "mat_b: a matrix of another curve"),
                (dict(C=tall), "mat_c: n_rows = 60 > m = 48"),
                (dict(n_z=N_COLS - 1), "mat_a: n_z = 8 < n_cols = 9"),
                (dict(mm=44), "m = 44 is not a domain size"),
                (dict(A=stale), "mat_a: matrix handle %d: not a live handle" % stale.handle),
                (dict(blind=(1, 2, 3), A=stale), "not a live handle"),
            ]
            for kw, words in cases:
                with pytest.raises(libff_amd.AmdMsmError) as e:
                    run(**kw)
                assert e.value.code == BAD_ARG and words in err(), (kw, err())
            with pytest.raises(libff_amd.AmdMsmError, match="overlap") as e:
                engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, at(d_z, f.limbs * 8))
            assert e.value.code == BAD_ARG
            assert (d.down(d_h, (m + 1, f.limbs)) == SENTINEL).all() and (d.down(d_z, zr.shape) == zr).all()
            with pytest.raises(libff_amd.AmdMsmError, match="domain size"):
                engine.qap_witness_map(curve, *mats, zr, 44)
            # the context works afterwards
            run()
            assert f.ints(d.down(d_h, (m + 1, f.limbs)), False) == expected(curve, rows, m, None)
    finally:
        for mt in mats + [other, tall]:
            mt.free()


def test_phases(engine):
    """[0] the tables of powers (host entry: with the upload), [1] the kernels, [2] the host entry's download"""
    curve, rows, m = 0, 43, 48
    f = fm.field(curve)
    a, b, c, z = qm.random_system(curve, rows, N_COLS)
    zr = f.records(z, False)
    want = f.records(expected(curve, rows, m, blinding(curve)), False)
    mats = load(engine, curve, (a, b, c), False)
    try:
        with Dev(engine) as d:
            d_z, d_h = d.up(zr), d.buf((m + 1) * f.limbs * 8)
            engine.set_timing(True)
            last = engine.last_timing_ticket()
            assert (engine.qap_witness_map(curve, *mats, zr, m, blind=blinding(curve)) == want).all()
            ticket = engine.last_timing_ticket()
            t = engine.get_timings(ticket=ticket)
            print("host", ticket, t)
            assert ticket != last
            assert t["scatter_ms"] > 0 and t["count_ms"] > 0 and t["accumulate_ms"] > 0 and t["total_ms"] >= t["scatter_ms"], t
            last = ticket
            engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, d_h, blind=blinding(curve))
            assert (d.down(d_h, (m + 1, f.limbs)) == want).all()
            ticket = engine.last_timing_ticket()
            t = engine.get_timings(ticket=ticket)
            print("device", ticket, t)
            assert ticket != last
            assert t["scatter_ms"] > 0 and t["count_ms"] > 0 and t["accumulate_ms"] == 0, t
            engine.set_timing(False)
            engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, d_h, blind=blinding(curve))
            assert (d.down(d_h, (m + 1, f.limbs)) == want).all()
    finally:
        engine.set_timing(False)
        for mt in mats:
            mt.free()


def test_h_into_the_msm_without_a_host_copy(engine, port):
    """the H-query of a prover: qap_witness_map_device writes the buffer msm_device reads its scalars from"""
    g = gmodel.group_of(port, "alt_bn128_g1")
    curve, rows, m = g.curve, 60, 64
    f = fm.field(curve)
    a, b, c, z = qm.random_system(curve, rows, N_COLS)
    h = expected(curve, rows, m, None)
    n = m - 1                                   # the coefficients of H that a Groth16 H-query multiplies
    logs = [random.Random(11).randrange(1, g.r) for _ in range(n)]
    bases = g.records(logs)
    want = g.records([sum(x * y for x, y in zip(h[:n], logs)) % g.r])
    s = libff_amd.sizes(g.curve, g.group)
    mats = load(engine, curve, (a, b, c), False)
    try:
        with Dev(engine) as d:
            d_xyz, d_aff = d.up(bases), d.buf(n * s["affine_bytes"])
            d_z, d_h, d_out = d.up(f.records(z, False)), d.buf((m + 1) * f.limbs * 8), d.buf(s["g_bytes"])
            engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], multi_exp_base_form_special, n, d_aff)
            engine.qap_witness_map_device(curve, *mats, d_z, len(z), m, d_h)
            engine.msm_device(g.curve, g.group, d_aff, d_h, n, d_out, out_form=OUT_AFFINE)
            assert (d.down(d_out, (1, g.gl)) == want).all()
    finally:
        for mt in mats:
            mt.free()
