"""Transforms over libfqfft's step radix-2 domains and the division by Z on the device (Engine.fr_domain_fft,
Engine.fr_domain_divide_by_z and their device forms) against the integer model tests/fr_domain_model.py, record for
record: the shapes at which the fold and the merge change their path (S from 1 to B / 2, one column over many workgroups,
partial sums in one and in two further launches), both record forms, all six fields, cosets, the device entry's rules,
a whole quotient on a step domain, and the phases of a timed call."""
import ctypes

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm
from fr_dev import BAD_ARG, SENTINEL, UNSUPPORTED, Dev, at, hip_runtime

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402

SIX = [pytest.param(c, id=n) for c, n in fm.CURVES.items()]
_expected = {}


def expected(curve, m, g=1):
    """(a, A(g x_j)) for the random vector of the size, computed once"""
    key = (curve, m, g)
    if key not in _expected:
        a = fm.random_vector(curve, m, seed=5)
        _expected[key] = (a, dm.transform(curve, a, g))
    return _expected[key]


def both_ways(engine, curve, m, g=None, plain=False, tile_log2=0):
    f = fm.field(curve)
    a, want = expected(curve, m, g or 1)
    there = engine.fr_domain_fft(curve, f.records(a, plain), coset=g, plain=plain, tile_log2=tile_log2)
    assert f.ints(there, plain) == want, ("forward", curve, m, g, plain)
    back = engine.fr_domain_fft(curve, f.records(want, plain), inverse=True, coset=g, plain=plain, tile_log2=tile_log2)
    assert f.ints(back, plain) == a, ("inverse", curve, m, g, plain)


@pytest.mark.parametrize("m", [3, 5, 6, 12, 24])
def test_smallest_shapes(engine, m):
    """K = 2 and 4, S = 1 .. 8: against Horner's rule itself"""
    a, want = expected(0, m)
    assert want == dm.transform_horner(0, a)
    both_ways(engine, 0, m)


@pytest.mark.parametrize("curve", SIX)
def test_every_field_in_both_record_forms(engine, curve):
    for m in (6, (1 << 9) + (1 << 3)):
        for plain in (False, True):
            both_ways(engine, curve, m, plain=plain)


@pytest.mark.parametrize("m", [(1 << 12) + 1, (1 << 14) + 1, (1 << 11) + (1 << 10), (1 << 13) + (1 << 5), (1 << 14) + (1 << 9)],
                         ids=["S1_4_partial_rows", "S1_16_partial_rows", "K2_widest", "S32_rows_share_a_tile", "S512_lane_per_column"])
def test_fold_paths(engine, m):
    """one column across 4 and 16 workgroups, whose partial sums a further launch adds up; two rows of 2^10 columns and no
    partial sums; between them a tile of eight rows of 32 columns and a lane per column, both with partial sums"""
    both_ways(engine, 0, m)


def unit_response(curve, m, k, g):
    """A(g x_j) for A = X^k, every j, one product each: two geometric sequences"""
    f = fm.field(curve)
    B, S = dm.shape(curve, m)
    w, r = f.root(2 * B), f.r
    out, x, q = [], pow(g, k, r), pow(w, 2 * k, r)
    for _ in range(B):
        out.append(x)
        x = x * q % r
    x, q = pow(g * w, k, r), pow(f.root(S), k, r)
    for _ in range(S):
        out.append(x)
        x = x * q % r
    return out


def test_two_levels_of_partial_sums(engine):
    """2^19 + 2^8: 2^11 rows of 256 columns leave 128 rows of partial sums, those 2, and a third launch the sums.  A
    unit vector in the last row against its closed form (plain records), and a dense vector there and back"""
    curve, m = 0, (1 << 19) + (1 << 8)
    f = fm.field(curve)
    g = fm.GENERATOR[curve]
    k = (1 << 19) - 3
    unit = np.zeros((m, f.limbs), dtype=np.uint64)
    unit[k, 0] = 1
    got = engine.fr_domain_fft(curve, unit, coset=g, plain=True)
    assert (got == f.records(unit_response(curve, m, k, g), True)).all()
    dense = np.random.default_rng(19).integers(0, 1 << 60, size=(m, f.limbs), dtype=np.uint64)   # below 2^252 < r
    for gg in (None, g):
        there = engine.fr_domain_fft(curve, dense, coset=gg)
        assert (there != dense).any()
        assert (engine.fr_domain_fft(curve, there, inverse=True, coset=gg) == dense).all()


def test_three_passes_and_a_single_pass(engine):
    m = (1 << 9) + (1 << 4)
    assert libff_amd.plan_fr_fft(0, 1 << 9, 4)["passes"] == 3 and libff_amd.plan_fr_fft(0, 1 << 4, 4)["passes"] == 1
    both_ways(engine, 0, m, tile_log2=4)
    both_ways(engine, 4, m, tile_log2=4, plain=True)


@pytest.mark.parametrize("m", [24, (1 << 12) + (1 << 4)])
def test_coset(engine, m):
    for curve in (0, 4):
        g = libff_amd.fr_multiplicative_generator(curve)
        assert g == fm.GENERATOR[curve]
        both_ways(engine, curve, m, g=g)
    both_ways(engine, 2, m, g=fm.GENERATOR[2], plain=True)


def test_large_default_tile(engine):
    """2^17 + 2^9: a unit vector against its closed form out[j] = (g x_j)^k, and a dense round trip"""
    curve, m = 0, (1 << 17) + (1 << 9)
    f = fm.field(curve)
    g = fm.GENERATOR[curve]
    assert unit_response(curve, 24, 17, g) == [pow(g * x % f.r, 17, f.r) for x in dm.elements(curve, 24)]
    for k, gg in (((1 << 17) + 77, None), ((1 << 16) + 5, g)):
        unit = np.zeros((m, f.limbs), dtype=np.uint64)
        unit[k] = f.records([1], False)[0]
        got = engine.fr_domain_fft(curve, unit, coset=gg)
        assert (got == f.records(unit_response(curve, m, k, gg or 1), False)).all()
    dense = f.records(fm.random_vector(curve, m, seed=9), False)
    for gg in (None, g):
        there = engine.fr_domain_fft(curve, dense, coset=gg)
        assert (there != dense).any()
        assert (engine.fr_domain_fft(curve, there, inverse=True, coset=gg) == dense).all()


def test_basic_domain_through_the_domain_entry(engine):
    curve, m = 1, 1 << 10
    f = fm.field(curve)
    g = fm.GENERATOR[curve]
    recs = f.records(fm.random_vector(curve, m, seed=3), False)
    assert libff_amd.fr_domain(curve, m)["kind"] == libff_amd.DOMAIN_BASIC_RADIX2
    for kw in ({}, {"coset": g}, {"inverse": True}, {"inverse": True, "coset": g}):
        assert (engine.fr_domain_fft(curve, recs, **kw) == engine.fr_fft(curve, recs, **kw)).all(), kw


@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(5, id="mnt6")])
def test_device_entry(engine, curve):
    f = fm.field(curve)
    rec = f.limbs * 8
    m = (1 << 9) + (1 << 6)
    a, want = expected(curve, m)
    want = f.records(want, False)
    hip = hip_runtime()
    with Dev(engine) as d:
        d_in = d.up(f.records(a, False))
        d_out = d.up(np.full((m + 4, f.limbs), SENTINEL, dtype=np.uint64))
        engine.fr_domain_fft_device(curve, d_in, m, at(d_out, 2 * rec))
        got = d.down(d_out, (m + 4, f.limbs))
        assert (got[2:-2] == want).all() and (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        assert (d.down(d_in, (m, f.limbs)) == f.records(a, False)).all()
        # out of place back again, behind the sentinels
        d_back = d.up(np.full((m + 4, f.limbs), SENTINEL, dtype=np.uint64))
        engine.fr_domain_fft_device(curve, at(d_out, 2 * rec), m, at(d_back, 2 * rec), inverse=True)
        got = d.down(d_back, (m + 4, f.limbs))
        assert (got[2:-2] == f.records(a, False)).all() and (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
        # a partial overlap is refused with nothing written
        h_in = d.down(d_in, (m, f.limbs))
        small = 24
        for src, dst in ((d_in, at(d_in, rec)), (at(d_in, rec), d_in)):
            with pytest.raises(libff_amd.AmdMsmError, match="overlap"):
                engine.fr_domain_fft_device(curve, src, small, dst)
            with pytest.raises(libff_amd.AmdMsmError, match="overlap"):
                engine.fr_domain_divide_by_z_device(curve, small, src, dst, coset=fm.GENERATOR[curve])
        assert (d.down(d_in, (m, f.limbs)) == h_in).all()
        # in place, on a stream of the caller's, there and back
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        try:
            engine.fr_domain_fft_device(curve, d_in, m, d_in, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
            assert (d.down(d_in, (m, f.limbs)) == want).all()
            engine.fr_domain_fft_device(curve, d_in, m, d_in, inverse=True, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
        finally:
            assert hip.hipStreamDestroy(stream) == 0
        assert (d.down(d_in, (m, f.limbs)) == h_in).all()


def test_refusals_with_a_context(engine):
    f = fm.field(0)
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    recs = f.records(fm.random_vector(0, 7, seed=1), False)
    out = np.full_like(recs, SENTINEL)
    with pytest.raises(libff_amd.AmdMsmError, match=r"m = 7 .* 8 ") as e:
        engine.fr_domain_fft(0, recs, out=out)
    assert e.value.code == BAD_ARG and (out == SENTINEL).all()
    # MNT6 above its 2-adicity: libfqfft would go on to a geometric domain, which is left out
    m = (1 << 17) + 1
    with Dev(engine) as d:
        d_buf = d.up(np.full((4, 5), SENTINEL, dtype=np.uint64))
        with pytest.raises(libff_amd.AmdMsmError, match="geometric") as e:
            engine.fr_domain_fft_device(5, d_buf, m, d_buf)
        assert e.value.code == UNSUPPORTED
        with pytest.raises(libff_amd.AmdMsmError, match="extended") as e:
            engine.fr_domain_fft_device(5, d_buf, 1 << 18, d_buf)
        assert e.value.code == UNSUPPORTED
        assert (d.down(d_buf, (4, 5)) == SENTINEL).all()
    # the division on the domain itself, or on a coset that meets it
    recs = f.records(fm.random_vector(0, 24, seed=1), False)
    out = np.full_like(recs, SENTINEL)
    for g in (f.root(32), 1, f.root(16), f.root(2)):
        with pytest.raises(libff_amd.AmdMsmError, match="zero") as e:
            engine.fr_domain_divide_by_z(0, recs, coset=g, out=out)
        assert e.value.code == BAD_ARG and (out == SENTINEL).all(), g
    assert "coset" in err()


@pytest.mark.parametrize("m", [24, (1 << 12) + 1, (1 << 11) + (1 << 10), 1 << 10])
def test_divide_by_z(engine, m):
    for curve, plain in ((0, False), (4, True)):
        f = fm.field(curve)
        g = fm.GENERATOR[curve]
        v = fm.random_vector(curve, m, seed=7)
        want = dm.divide_by_z(curve, v, g)
        got = engine.fr_domain_divide_by_z(curve, f.records(v, plain), coset=g, plain=plain)
        assert f.ints(got, plain) == want, (curve, m)
    with Dev(engine) as d:   # the device entry in place, behind and in front of sentinels
        f = fm.field(0)
        rec = f.limbs * 8
        v = fm.random_vector(0, m, seed=7)
        buf = np.full((m + 2, f.limbs), SENTINEL, dtype=np.uint64)
        buf[1:-1] = f.records(v, False)
        d_buf = d.up(buf)
        engine.fr_domain_divide_by_z_device(0, m, at(d_buf, rec), at(d_buf, rec), coset=fm.GENERATOR[0])
        got = d.down(d_buf, buf.shape)
        assert f.ints(got[1:-1], False) == dm.divide_by_z(0, v, fm.GENERATOR[0])
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()


def _poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % r for v in out]


@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4")])
def test_quotient_on_a_step_domain(engine, curve):
    """h = (A B - C) / Z with every step on the device: three inverse transforms, three coset transforms, the pointwise
    a b - c, the division by Z on the coset, the inverse coset transform"""
    m = (1 << 10) + (1 << 4)
    f = fm.field(curve)
    r, g = f.r, libff_amd.fr_multiplicative_generator(curve)
    a, b = fm.random_vector(curve, m, 1), fm.random_vector(curve, m, 2)
    c = [x * y % r for x, y in zip(a, b)]
    with Dev(engine) as d:
        bufs = [d.up(f.records(v, False)) for v in (a, b, c)]
        for p in bufs:
            engine.fr_domain_fft_device(curve, p, m, p, inverse=True)
            engine.fr_domain_fft_device(curve, p, m, p, coset=g)
        d_h = d.buf(m * f.limbs * 8)
        engine.fr_muladd_device(curve, m, bufs[0], bufs[1], d_h, d_c=bufs[2])
        engine.fr_domain_divide_by_z_device(curve, m, d_h, d_h, coset=g)
        engine.fr_domain_fft_device(curve, d_h, m, d_h, inverse=True, coset=g)
        h = f.ints(d.down(d_h, (m, f.limbs)), False)
    A, B, C = (dm.interpolate(curve, v) for v in (a, b, c))
    lhs = _poly_mul(A, B, r)
    for i, x in enumerate(C):
        lhs[i] = (lhs[i] - x) % r
    assert h[m - 1] == 0
    assert lhs == _poly_mul(h[:m - 1], _dense_z(curve, m), r)


def _dense_z(curve, m):
    z = [0] * (m + 1)
    for i, coef in dm.z_terms(curve, m):
        z[i] = (z[i] + coef) % fm.field(curve).r
    return z


def test_phases(engine):
    """[0] the powers (host entry: with the upload), [1] the kernels, [2] the download of the host entry alone; a ticket
    per call; and the same records with timing off"""
    curve, m = 1, (1 << 11) + (1 << 7)
    f = fm.field(curve)
    g = fm.GENERATOR[curve]
    rec = f.limbs * 8
    a, want = expected(curve, m, g)
    recs, want = f.records(a, False), f.records(want, False)
    quot = f.records(dm.divide_by_z(curve, a, g), False)
    with Dev(engine) as d:
        d_in, d_out = d.up(recs), d.buf(m * rec)
        cases = [
            ("fft", lambda: engine.fr_domain_fft(curve, recs, coset=g),
             lambda: (engine.fr_domain_fft_device(curve, d_in, m, d_out, coset=g), d.down(d_out, (m, f.limbs)))[1], want),
            ("inverse", lambda: engine.fr_domain_fft(curve, want, coset=g, inverse=True),
             lambda: (engine.fr_domain_fft_device(curve, d.up(want), m, d_out, coset=g, inverse=True), d.down(d_out, (m, f.limbs)))[1], recs),
            ("divide", lambda: engine.fr_domain_divide_by_z(curve, recs, coset=g),
             lambda: (engine.fr_domain_divide_by_z_device(curve, m, d_in, d_out, coset=g), d.down(d_out, (m, f.limbs)))[1], quot),
        ]
        try:
            engine.set_timing(True)
            last = engine.last_timing_ticket()
            for name, host, device, expect in cases:
                assert (host() == expect).all(), name
                ticket = engine.last_timing_ticket()
                t = engine.get_timings(ticket=ticket)
                print(name, "host", ticket, t)
                assert ticket != last, name
                assert t["scatter_ms"] > 0 and t["count_ms"] > 0 and t["accumulate_ms"] > 0, (name, t)
                assert t["total_ms"] >= t["scatter_ms"], (name, t)
                last = ticket
                assert (device() == expect).all(), name
                ticket = engine.last_timing_ticket()
                t = engine.get_timings(ticket=ticket)
                print(name, "device", ticket, t)
                assert ticket != last, name
                assert t["scatter_ms"] > 0 and t["count_ms"] >= 0 and t["accumulate_ms"] == 0, (name, t)
                last = ticket
            engine.set_timing(False)
            for name, host, device, expect in cases:
                assert (host() == expect).all() and (device() == expect).all(), name
        finally:
            engine.set_timing(False)
