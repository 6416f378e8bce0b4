"""Scans and batch inversion over Fr vectors on the device (Engine.fr_scan / fr_scan_device, fr_batch_invert /
fr_batch_invert_device), all six scalar fields, the tiled path and the one-lane path behind AMDMSM_FR_SCAN_NAIVE=1.
Expected values come from tests/fr_scan_model.py -- Python integers, the recurrence as a loop and the inverse as a power
-- and everything is compared record for record.  Nothing here knows how a tile is cut: the sizes come from what
libff_amd.plan_fr_scan reports (the smallest tile T0, the tiles S0 of a spine step, the default tile)."""
import ctypes
import random

import numpy as np
import pytest

import fr_scan_model as model
import group_fft_model as gmodel
from fr_dev import BAD_ARG, FOUR, OK, SENTINEL, TOO_LARGE, UNSUPPORTED, Dev, at, env_path, hip_runtime, poly_eval

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, fr_inverse, multi_exp_base_form_special, plan_fr_scan  # noqa: E402

CURVES = sorted(model.CURVES)
IDS = [model.CURVES[c] for c in CURVES]
PATHS = [pytest.param(False, id="tiled"), pytest.param(True, id="naive")]
# which operands a scan is given: (a vector, a_const, b vector)
COMBOS = [(True, False, False), (True, False, True), (False, True, False), (False, True, True), (False, False, True)]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]   # (reverse, exclusive)


def path(naive):
    """the environment of a call: AMDMSM_FR_SCAN_NAIVE is read per call"""
    return env_path("AMDMSM_FR_SCAN_NAIVE", naive)


def geometry(curve):
    """(smallest tile_log2, T0, S0, default tile) from the plan"""
    p = plan_fr_scan(curve, 0)
    lo = p["tile_min"]
    small = plan_fr_scan(curve, 0, tile_log2=lo)
    assert small["tile"] == 1 << lo <= 1 << 8 and small["tile"] * small["spine_step"] <= 1 << 17
    return lo, small["tile"], small["spine_step"], p["tile"]


_vecs = {}


def vectors(curve, n, plain):
    """(a, b, records of a, records of b): n random values each, with 1, r - 1 and small values among them; computed once
    per (curve, n, form) and never changed"""
    key = (curve, n, plain)
    if key not in _vecs:
        f = model.field(curve)
        a, b = model.random_vector(curve, n, seed=1), model.random_vector(curve, n, seed=2)
        for i in range(0, n, 7):
            a[i] = (1, f.r - 1, 2, f.r - 2)[(i // 7) % 4]
        for i in range(3, n, 11):
            b[i] = (0, 1, f.r - 1)[(i // 11) % 3]
        _vecs[key] = (a, b, f.records(a, plain) if n else np.zeros((0, f.limbs), dtype=np.uint64),
                      f.records(b, plain) if n else np.zeros((0, f.limbs), dtype=np.uint64))
    return _vecs[key]


def device_scan(engine, d, curve, n, ra, rb, *, a_const=None, init=None, reverse=False, exclusive=False, plain=False, tile_log2=0,
                total=True, stream=None):
    """one device call between sentinels: (out records, total record or None)"""
    f = model.field(curve)
    rec = f.limbs * 8
    d_a = None if ra is None else d.up(ra)
    d_b = None if rb is None else d.up(rb)
    d_out = d.up(np.full((n + 2, f.limbs), SENTINEL, dtype=np.uint64))
    d_tot = d.up(np.full((3, f.limbs), SENTINEL, dtype=np.uint64))
    engine.fr_scan_device(curve, n, at(d_out, rec), d_a, d_b, a_const=a_const, init=init, d_total=at(d_tot, rec) if total else None,
                          reverse=reverse, exclusive=exclusive, plain=plain, tile_log2=tile_log2, stream=stream)
    if stream is not None:
        assert hip_runtime().hipStreamSynchronize(stream) == 0
    out, tot = d.down(d_out, (n + 2, f.limbs)), d.down(d_tot, (3, f.limbs))
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "d_out: written outside its n records"
    assert (tot[0] == SENTINEL).all() and (tot[2] == SENTINEL).all(), "d_total: written outside its record"
    if not total:
        assert (tot[1] == SENTINEL).all()
    return out[1:-1], tot[1] if total else None


def check_scan(engine, curve, n, combo, flags, *, plain=False, tile_log2=0, init="given", total=True, values=None):
    """one case on the device against the model"""
    f = model.field(curve)
    has_a, has_c, has_b = combo
    reverse, exclusive = flags
    a, b, ra, rb = vectors(curve, n, plain) if values is None else values
    z = model.random_vector(curve, 1, seed=77)[0]
    ini = None if init == "default" else model.random_vector(curve, 1, seed=78)[0]
    want, wtot = model.scan(f.r, n, a if has_a else None, b if has_b else None, z if has_c else None, ini, reverse, exclusive)
    with Dev(engine) as d:
        out, tot = device_scan(engine, d, curve, n, ra if has_a else None, rb if has_b else None, a_const=z if has_c else None, init=ini,
                               reverse=reverse, exclusive=exclusive, plain=plain, tile_log2=tile_log2, total=total)
    what = (model.CURVES[curve], n, combo, flags, plain, tile_log2, init)
    assert (out == (f.records(want, plain) if n else out)).all(), what
    if total:
        assert (tot == f.records([wtot], plain)[0]).all(), what


# ---- scans ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_scan_all_fields_both_forms(engine, curve, naive):
    lo, T0, _, _ = geometry(curve)
    k = 0
    with path(naive):
        for plain in (False, True):
            for n in (0, 1, 2, 63, 64, 65):
                for combo in COMBOS:
                    k += 1
                    check_scan(engine, curve, n, combo, FLAGS[k % 4], plain=plain, tile_log2=lo, init=("given", "default")[k % 2],
                               total=k % 3 != 0)


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_scan_every_combination_around_a_tile(engine, curve, naive):
    """a, a_const or neither with b or none, forward and reverse, inclusive and exclusive, init given and defaulted,
    d_total given and NULL: at one below, at and one above the smallest tile, at two tiles and a record, at the default
    tile's edges and at three of them and five records"""
    lo, T0, _, Td = geometry(curve)
    with path(naive):
        for tl, sizes in ((lo, (T0 - 1, T0, T0 + 1, 2 * T0 + 1)), (0, (Td - 1, Td, Td + 1, 3 * Td + 5))):
            for i, n in enumerate(sizes):
                for j, combo in enumerate(COMBOS):
                    for k, flags in enumerate(FLAGS):
                        full = n in (T0 + 1, 3 * Td + 5)   # every flag pair there, one in turn at the other sizes
                        if not full and k != (i + j) % 4:
                            continue
                        check_scan(engine, curve, n, combo, flags, plain=(i + j + k) % 2 == 1, tile_log2=tl,
                                   init=("given", "default")[(j + k) % 2], total=(i + k) % 2 == 0)


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_scan_across_the_spine_steps(engine, curve, naive):
    """S0 T0 - 1, S0 T0 and S0 T0 + 1 records at the smallest tile: the spine's carry from one step to the next"""
    lo, T0, S0, _ = geometry(curve)
    assert S0 * T0 + 1 <= (1 << 17) + 1
    cases = [((True, False, True), (False, False)), ((True, False, False), (True, True)), ((False, True, True), (True, True))]
    with path(naive):
        for i, n in enumerate((S0 * T0 - 1, S0 * T0, S0 * T0 + 1)):
            combo, flags = cases[i]
            check_scan(engine, curve, n, combo, flags, tile_log2=lo, init=("given", "default")[i % 2])
        check_scan(engine, curve, S0 * T0 + 1, (False, False, True), (False, True), tile_log2=lo, plain=True)
        # the larger tiles, whose spine lanes take several aggregates each: as many tiles as 2^17 records make
        for tl in range(lo + 1, plan_fr_scan(curve, 0)["tile_max"] + 1):
            p = plan_fr_scan(curve, (1 << 17) - 3, tile_log2=tl)
            assert p["spine_step"] > S0
            check_scan(engine, curve, (1 << 17) - 3, (True, False, True), (tl % 2 == 0, tl % 2 == 1), tile_log2=tl)


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_scan_special_operands(engine, curve, naive):
    """r - 1 throughout; a zero among the a_i, behind which only b counts; every a_i one"""
    f = model.field(curve)
    r = f.r
    lo, T0, _, _ = geometry(curve)
    n = 2 * T0 + 1
    with path(naive):
        for plain in (False, True):
            top = [r - 1] * n
            rt = f.records(top, plain)
            for combo in ((True, False, True), (True, False, False), (False, False, True)):
                for flags in ((False, False), (True, True)):
                    check_scan(engine, curve, n, combo, flags, plain=plain, tile_log2=lo, values=(top, top, rt, rt))
            a, b, _, rb = vectors(curve, n, plain)
            for zero_at in (0, T0 - 1, T0, n - 1):
                az = list(a)
                az[zero_at] = 0
                vals = (az, b, f.records(az, plain), rb)
                check_scan(engine, curve, n, (True, False, True), (False, False), plain=plain, tile_log2=lo, values=vals)
                check_scan(engine, curve, n, (True, False, False), (False, True), plain=plain, tile_log2=lo, values=vals)
                # behind the zero nothing of what came before it is left: the scan starts again from b at the zero
                want, _ = model.scan(r, n, az, b, init=5)
                tail, _ = model.scan(r, n - zero_at - 1, az[zero_at + 1:], b[zero_at + 1:], init=b[zero_at])
                assert want[zero_at + 1:] == tail
            ones = [1] * n
            vals = (ones, b, f.records(ones, plain), rb)
            check_scan(engine, curve, n, (True, False, True), (True, False), plain=plain, tile_log2=lo, values=vals)
            check_scan(engine, curve, n, (True, False, False), (False, False), plain=plain, tile_log2=lo, values=vals)


def test_host_entries_and_timings(engine):
    curve = 1
    f = model.field(curve)
    _, _, _, Td = geometry(curve)
    n = Td + 3
    a, b, ra, rb = vectors(curve, n, False)
    for naive in (False, True):
        with path(naive):
            out, tot = engine.fr_scan(curve, ra, rb, init=9)
            want, wtot = model.scan(f.r, n, a, b, init=9)
            assert (out == f.records(want, False)).all() and (tot == f.records([wtot], False)[0]).all()
            out, tot = engine.fr_scan(curve, None, rb, a_const=3, reverse=True, exclusive=True)
            want, wtot = model.scan(f.r, n, None, b, a_const=3, reverse=True, exclusive=True)
            assert (out == f.records(want, False)).all() and (tot == f.records([wtot], False)[0]).all()
            out, tot = engine.fr_scan(curve, np.zeros((0, f.limbs), dtype=np.uint64), init=4, plain=True)
            assert out.shape == (0, f.limbs) and f.ints([tot], True) == [4]
            inv, zeros = engine.fr_batch_invert(curve, ra)
            winv, wz = model.invert(f.r, a)
            assert zeros == wz and (inv == f.records(winv, False)).all()
            inv, zeros = engine.fr_batch_invert(curve, np.zeros((0, f.limbs), dtype=np.uint64))
            assert zeros == 0 and inv.shape == (0, f.limbs)
    engine.set_timing(True)
    try:
        engine.fr_scan(curve, ra, rb)
        t = engine.get_timings()
        assert t["scatter_ms"] > 0 and t["total_ms"] >= t["scatter_ms"] and t["count_ms"] >= 0 and t["accumulate_ms"] >= 0
    finally:
        engine.set_timing(False)


# ---- batch inversion -----------------------------------------------------------------------------------------------------
def device_invert(engine, d, curve, recs, *, plain=False, tile_log2=0, count=True, in_place=False, stream=None):
    f = model.field(curve)
    rec, n = f.limbs * 8, recs.shape[0]
    d_cnt = d.up(np.array([SENTINEL, 12345, SENTINEL], dtype=np.uint64))   # the caller need not clear it
    if in_place:
        d_out = d.up(np.concatenate([np.full((1, f.limbs), SENTINEL, dtype=np.uint64), recs, np.full((1, f.limbs), SENTINEL, dtype=np.uint64)]))
        d_in = at(d_out, rec)
    else:
        d_in, d_out = d.up(recs), d.up(np.full((n + 2, f.limbs), SENTINEL, dtype=np.uint64))
    engine.fr_batch_invert_device(curve, n, d_in, at(d_out, rec), at(d_cnt, 8) if count else None, plain=plain, tile_log2=tile_log2,
                                  stream=stream)
    if stream is not None:
        assert hip_runtime().hipStreamSynchronize(stream) == 0
    out, cnt = d.down(d_out, (n + 2, f.limbs)), d.down(d_cnt, (3,))
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "d_out: written outside its n records"
    assert cnt[0] == SENTINEL and cnt[2] == SENTINEL and (count or cnt[1] == 12345)
    return out[1:-1], int(cnt[1]) if count else None


def check_invert(engine, curve, values, *, plain=False, tile_log2=0, count=True, in_place=False):
    f = model.field(curve)
    want, zeros = model.invert(f.r, values)
    recs = f.records(values, plain) if values else np.zeros((0, f.limbs), dtype=np.uint64)
    with Dev(engine) as d:
        out, cnt = device_invert(engine, d, curve, recs, plain=plain, tile_log2=tile_log2, count=count, in_place=in_place)
    what = (model.CURVES[curve], len(values), plain, tile_log2)
    assert (out == (f.records(want, plain) if values else out)).all(), what
    if count:
        assert cnt == zeros, what


def invert_values(curve, n):
    """random values with 1, r - 1 and a few zeros among them.  Above 4096 records the values are drawn from the first
    499 of them, in an order that does not repeat with any tile, so that the model takes 499 powers and not n"""
    a = list(vectors(curve, n, False)[0])
    if n > 4096:
        a = [a[(i * i + i // 3) % 499] for i in range(n)]
    for i in range(5, n, 13):
        a[i] = 0
    return a


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_invert_all_fields_both_forms(engine, curve, naive):
    lo, _, _, _ = geometry(curve)
    with path(naive):
        for plain in (False, True):
            for k, n in enumerate((0, 1, 2, 63, 64, 65)):
                check_invert(engine, curve, invert_values(curve, n), plain=plain, tile_log2=lo, count=k % 2 == 0, in_place=k % 3 == 0)


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_invert_at_the_edges(engine, curve, naive):
    lo, T0, S0, Td = geometry(curve)
    with path(naive):
        for k, n in enumerate((T0 - 1, T0, T0 + 1, 2 * T0 + 1)):
            check_invert(engine, curve, invert_values(curve, n), plain=k % 2 == 1, tile_log2=lo, in_place=k % 2 == 0)
        for k, n in enumerate((Td - 1, Td, Td + 1, 3 * Td + 5)):
            check_invert(engine, curve, invert_values(curve, n), plain=k % 2 == 0, count=k != 1)
        for k, n in enumerate((S0 * T0 - 1, S0 * T0, S0 * T0 + 1)):
            check_invert(engine, curve, invert_values(curve, n), tile_log2=lo, in_place=k == 1)
        for tl in range(lo + 1, plan_fr_scan(curve, 0)["tile_max"] + 1):   # several aggregates to a lane of the spine
            check_invert(engine, curve, invert_values(curve, (1 << 17) - 3), tile_log2=tl)


@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR)
def test_invert_zeros_are_counted_and_stay_zero(engine, curve, naive):
    """a zero at index 0, at the last index, on both sides of a tile edge, a whole tile of zeros, every record zero"""
    f = model.field(curve)
    lo, T0, _, _ = geometry(curve)
    n = 3 * T0 + 7
    base = [v or 1 for v in vectors(curve, n, False)[0]]
    assert 0 not in base

    def with_zeros(at_):
        v = list(base)
        for i in at_:
            v[i] = 0
        return v

    with path(naive):
        for k, zeros in enumerate(([0], [n - 1], [T0 - 1, T0], [2 * T0 - 1], [2 * T0], list(range(T0, 2 * T0)), [0, n - 1, T0],
                                   list(range(n)))):
            check_invert(engine, curve, with_zeros(zeros), plain=k % 2 == 1, tile_log2=lo, count=True, in_place=k % 3 == 1)
        check_invert(engine, curve, with_zeros([0, T0]), tile_log2=lo, count=False)
        # ones and r - 1 are their own inverses
        check_invert(engine, curve, [1, f.r - 1] * T0 + [1], tile_log2=lo)
        # x * (1 / x) = 1 by the product step of the library
        ones = f.records([1] * n, False)
        with Dev(engine) as d:
            d_x, d_inv, d_one = d.up(f.records(base, False)), d.buf(n * f.limbs * 8), d.buf(n * f.limbs * 8)
            engine.fr_batch_invert_device(curve, n, d_x, d_inv, None, tile_log2=lo)
            engine.fr_muladd_device(curve, n, d_x, d_inv, d_one)
            assert (d.down(d_one, (n, f.limbs)) == ones).all()


# ---- placement and streams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("naive", PATHS)
@pytest.mark.parametrize("curve", FOUR[:3])
def test_in_place_on_each_alias(engine, curve, naive):
    f = model.field(curve)
    lo, T0, _, Td = geometry(curve)
    with path(naive):
        for tl, n in ((lo, 2 * T0 + 1), (0, Td + 9)):
            a, b, ra, rb = vectors(curve, n, False)
            for alias in ("a", "b"):
                for flags in ((False, False), (True, True)):
                    want, wtot = model.scan(f.r, n, a, b, init=6, reverse=flags[0], exclusive=flags[1])
                    with Dev(engine) as d:
                        d_a, d_b, d_t = d.up(ra), d.up(rb), d.buf(f.limbs * 8)
                        d_out = d_a if alias == "a" else d_b
                        engine.fr_scan_device(curve, n, d_out, d_a, d_b, init=6, d_total=d_t, reverse=flags[0], exclusive=flags[1], tile_log2=tl)
                        assert (d.down(d_out, (n, f.limbs)) == f.records(want, False)).all(), (alias, flags, n)
                        assert (d.down(d_t, (1, f.limbs)) == f.records([wtot], False)).all()
                        other = d.down(d_b if alias == "a" else d_a, (n, f.limbs))
                        assert (other == (rb if alias == "a" else ra)).all(), "the other operand is read only"
            # one vector alone, in place
            for combo_a in (True, False):
                want, _ = model.scan(f.r, n, a if combo_a else None, None if combo_a else b, exclusive=True)
                with Dev(engine) as d:
                    d_v = d.up(ra if combo_a else rb)
                    engine.fr_scan_device(curve, n, d_v, d_v if combo_a else None, None if combo_a else d_v, exclusive=True, tile_log2=tl)
                    assert (d.down(d_v, (n, f.limbs)) == f.records(want, False)).all()


@pytest.mark.parametrize("naive", PATHS)
def test_callers_stream_and_two_streams(engine, naive):
    curve = 3
    f = model.field(curve)
    lo, T0, _, Td = geometry(curve)
    hip = hip_runtime()
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        with path(naive), Dev(engine) as d:
            n = 3 * T0 + 5
            a, b, ra, rb = vectors(curve, n, False)
            out, tot = device_scan(engine, d, curve, n, ra, rb, init=3, tile_log2=lo, stream=streams[0])
            want, wtot = model.scan(f.r, n, a, b, init=3)
            assert (out == f.records(want, False)).all() and (tot == f.records([wtot], False)[0]).all()
            inv, cnt = device_invert(engine, d, curve, ra, tile_log2=lo, stream=streams[1])
            winv, wz = model.invert(f.r, a)
            assert (inv == f.records(winv, False)).all() and cnt == wz
            # two calls on two streams, enqueued back to back
            m = Td + 1
            a2, b2, ra2, rb2 = vectors(curve, m, False)
            d_a, d_b, d_a2 = d.up(ra), d.up(rb), d.up(ra2)
            o1, o2, o3 = d.buf(n * f.limbs * 8), d.buf(m * f.limbs * 8), d.buf(n * f.limbs * 8)
            engine.fr_scan_device(curve, n, o1, d_a, d_b, reverse=True, tile_log2=lo, stream=streams[0])
            engine.fr_batch_invert_device(curve, m, d_a2, o2, None, stream=streams[1])
            engine.fr_scan_device(curve, n, o3, None, d_b, a_const=7, exclusive=True, stream=streams[1])
            for s in streams:
                assert hip.hipStreamSynchronize(s) == 0
            assert (d.down(o1, (n, f.limbs)) == f.records(model.scan(f.r, n, a, b, reverse=True)[0], False)).all()
            assert (d.down(o2, (m, f.limbs)) == f.records(model.invert(f.r, a2)[0], False)).all()
            assert (d.down(o3, (n, f.limbs)) == f.records(model.scan(f.r, n, None, b, a_const=7, exclusive=True)[0], False)).all()
    finally:
        for s in streams:
            assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("naive", PATHS)
def test_a_record_that_is_no_field_element(engine, naive):
    """a record >= r in the input: sentinels intact, and the outputs that do not depend on it as they should be"""
    curve = 0
    f = model.field(curve)
    lo, T0, _, _ = geometry(curve)
    n, bad = 3 * T0 + 2, T0 + 17
    a, b, ra, rb = vectors(curve, n, False)
    ra, rb = ra.copy(), rb.copy()
    ra[bad] = np.uint64(0xffffffffffffffff)
    with path(naive), Dev(engine) as d:
        out, _ = device_scan(engine, d, curve, n, ra, rb, init=2, tile_log2=lo)
        want = f.records(model.scan(f.r, n, a, b, init=2)[0], False)
        assert (out[:bad] == want[:bad]).all()
        out, _ = device_scan(engine, d, curve, n, ra, rb, init=2, tile_log2=lo, reverse=True, exclusive=True)
        want = f.records(model.scan(f.r, n, a, b, init=2, reverse=True, exclusive=True)[0], False)
        assert (out[bad:] == want[bad:]).all()   # exclusive: record `bad` itself holds the value that enters it
        rb[bad] = np.uint64(0xffffffffffffffff)
        out, _ = device_scan(engine, d, curve, n, None, rb, tile_log2=lo)
        want = f.records(model.scan(f.r, n, None, b)[0], False)
        assert (out[:bad] == want[:bad]).all()
        device_invert(engine, d, curve, ra, tile_log2=lo)   # every output depends on it: the sentinels are the check


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", FOUR[:3])
def test_refused_calls_leave_the_output_alone(engine, curve):
    """every refusal of the four entries, with a context: the code, what amdmsm_last_error names, the output untouched"""
    f = model.field(curve)
    rec, n = f.limbs * 8, 8
    lo = plan_fr_scan(curve, 0)["tile_min"]
    hi = plan_fr_scan(curve, 0)["tile_max"]
    a, b, ra, rb = vectors(curve, n, True)
    o, bad_opts = engine._opts(scalars_plain=True), engine._opts(scalars_plain=True)
    bad_opts.struct_size += 8
    ptr = lambda v: None if v is None else v.ctypes.data_as(ctypes.c_void_p)
    err = lambda: engine.lib.amdmsm_last_error(engine.h)
    sz = ctypes.c_size_t
    one, big = f.records([1], True)[0], np.frombuffer(f.r.to_bytes(rec, "little"), dtype="<u8").astype(np.uint64)
    L = engine.lib

    def scan_rules(call, va, vb, dst, tot, read):
        """the rules the host and the device entry share"""
        def refused(code, word, *args, **kw):
            assert call(*args, **kw) == code and word in err(), (word, err())
            assert (read() == SENTINEL).all(), word

        refused(UNSUPPORTED, b"curve", 6, n, va, None, vb, None, 0, 0)
        refused(BAD_ARG, b"struct_size", curve, n, va, None, vb, None, 0, 0, opts=bad_opts)
        refused(TOO_LARGE, b"2^28", curve, (1 << 28) + 1, va, None, vb, None, 0, 0)
        refused(BAD_ARG, b"flags", curve, n, va, None, vb, None, 4, 0)
        refused(BAD_ARG, b"flags", curve, n, va, None, vb, None, 0x100, 0)
        refused(BAD_ARG, b"a and a_const", curve, n, va, ptr(one), vb, None, 0, 0)
        refused(BAD_ARG, b"a and b", curve, n, None, None, None, None, 0, 0)
        refused(BAD_ARG, b"out", curve, n, va, None, vb, None, 0, 0, dst=None)
        refused(BAD_ARG, b"tile_log2", curve, n, va, None, vb, None, 0, lo - 1)
        refused(BAD_ARG, b"tile_log2", curve, n, va, None, vb, None, 0, hi + 1)
        refused(BAD_ARG, b"a_const", curve, n, None, ptr(big), vb, None, 0, 0)
        refused(BAD_ARG, b"init", curve, n, va, None, vb, ptr(big), 0, 0)
        assert call(curve, n, va, None, vb, ptr(one), 3, lo) == OK

    out, tot = np.full((n, f.limbs), SENTINEL, dtype=np.uint64), np.full(f.limbs, SENTINEL, dtype=np.uint64)

    def host(c, n_, va, ac, vb, ini, flags, tl, opts=o, dst=ptr(out)):
        return L.amdmsm_fr_scan(engine.h, c, sz(n_), va, ac, vb, ini, flags, tl, ctypes.byref(opts), dst, ptr(tot))

    scan_rules(host, ptr(ra), ptr(rb), ptr(out), ptr(tot), lambda: np.concatenate([out.ravel(), tot]))
    want, wtot = model.scan(f.r, n, a, b, init=1, reverse=True, exclusive=True)
    assert (out == f.records(want, True)).all() and (tot == f.records([wtot], True)[0]).all()

    inv_out, cnt = np.full((n, f.limbs), SENTINEL, dtype=np.uint64), ctypes.c_uint64(SENTINEL)
    hinv = lambda c, n_, v, opts=o, dst=ptr(inv_out): L.amdmsm_fr_batch_invert(engine.h, c, sz(n_), v, ctypes.byref(opts), dst, ctypes.byref(cnt))
    untouched = lambda: (inv_out == SENTINEL).all() and cnt.value == SENTINEL
    assert hinv(6, n, ptr(ra)) == UNSUPPORTED and b"curve" in err() and untouched()
    assert hinv(curve, n, ptr(ra), opts=bad_opts) == BAD_ARG and b"struct_size" in err() and untouched()
    assert hinv(curve, (1 << 28) + 1, ptr(ra)) == TOO_LARGE and b"2^28" in err() and untouched()
    assert hinv(curve, n, None) == BAD_ARG and b"values" in err() and untouched()
    assert hinv(curve, n, ptr(ra), dst=None) == BAD_ARG and b"out" in err() and untouched()
    assert hinv(curve, n, ptr(ra)) == OK and cnt.value == model.invert(f.r, a)[1]
    assert (inv_out == f.records(model.invert(f.r, a)[0], True)).all()

    with Dev(engine) as d:
        d_a, d_b = d.up(ra), d.up(rb)
        d_out, d_tot = d.up(np.full((n, f.limbs), SENTINEL, dtype=np.uint64)), d.up(np.full((2, f.limbs), SENTINEL, dtype=np.uint64))
        read = lambda: np.concatenate([d.down(d_out, (n, f.limbs)).ravel(), d.down(d_tot, (2, f.limbs)).ravel()])

        def dev(c, n_, va, ac, vb, ini, flags, tl, opts=o, dst=d_out, total=d_tot):
            return L.amdmsm_fr_scan_device(engine.h, c, sz(n_), va, ac, vb, ini, flags, tl, ctypes.byref(opts), dst, total)

        scan_rules(dev, d_a, d_b, d_out, d_tot, read)
        assert (d.down(d_out, (n, f.limbs)) == f.records(want, True)).all()
        assert (d.down(d_tot, (1, f.limbs)) == f.records([wtot], True)).all()
        # the device entries' own rules: alignment and partial overlap
        d_big = d.up(np.full((4 * n, f.limbs), SENTINEL, dtype=np.uint64))
        engine.h2d(d_big, ra)
        before = d.down(d_big, (4 * n, f.limbs))
        for args, word in (((at(d_big, 4), None, d_b, None, 0, 0), b"d_a"), ((d_a, None, at(d_big, 4), None, 0, 0), b"d_b")):
            assert dev(curve, n, *args, dst=at(d_big, 2 * n * rec)) == BAD_ARG and word in err() and b"aligned" in err()
        assert dev(curve, n, d_a, None, d_b, None, 0, 0, dst=at(d_big, 4)) == BAD_ARG and b"d_out" in err() and b"aligned" in err()
        assert dev(curve, n, d_a, None, d_b, None, 0, 0, dst=at(d_big, 2 * n * rec), total=at(d_big, 4)) == BAD_ARG and b"d_total" in err()
        assert dev(curve, n, d_big, None, d_b, None, 0, 0, dst=at(d_big, 3 * rec)) == BAD_ARG and b"overlap" in err() and b"d_a" in err()
        assert dev(curve, n, d_a, None, d_big, None, 0, 0, dst=at(d_big, (n - 1) * rec)) == BAD_ARG and b"overlap" in err() and b"d_b" in err()
        assert dev(curve, n, d_a, None, d_b, None, 0, 0, dst=d_big, total=at(d_big, 2 * rec)) == BAD_ARG and b"d_total" in err()
        dinv = lambda n_, v, dst, c=None, tl=0, opts=o, cv=curve: L.amdmsm_fr_batch_invert_device(engine.h, cv, sz(n_), v, tl, ctypes.byref(opts), dst, c)
        assert dinv(n, d_a, at(d_big, 2 * n * rec), cv=6) == UNSUPPORTED and b"curve" in err()
        assert dinv(n, d_a, at(d_big, 2 * n * rec), opts=bad_opts) == BAD_ARG and b"struct_size" in err()
        assert dinv((1 << 28) + 1, d_a, at(d_big, 2 * n * rec)) == TOO_LARGE and b"2^28" in err()
        assert dinv(n, None, at(d_big, 2 * n * rec)) == BAD_ARG and b"values" in err()
        assert dinv(n, d_a, None) == BAD_ARG and b"out" in err()
        assert dinv(n, at(d_big, 4), at(d_big, 2 * n * rec)) == BAD_ARG and b"d_values" in err() and b"aligned" in err()
        assert dinv(n, d_a, at(d_big, 4)) == BAD_ARG and b"d_out" in err() and b"aligned" in err()
        assert dinv(n, d_a, at(d_big, 2 * n * rec), c=at(d_big, 4)) == BAD_ARG and b"d_zero_count" in err()
        assert dinv(n, d_a, at(d_big, 2 * n * rec), c=at(d_big, 2 * n * rec + 8)) == BAD_ARG and b"d_zero_count" in err()
        assert dinv(n, d_big, at(d_big, 2 * rec)) == BAD_ARG and b"overlap" in err()
        assert dinv(n, d_a, at(d_big, 2 * n * rec), tl=lo - 1) == BAD_ARG and b"tile_log2" in err()
        assert dinv(n, d_a, at(d_big, 2 * n * rec), tl=hi + 1) == BAD_ARG and b"tile_log2" in err()
        assert (d.down(d_big, (4 * n, f.limbs)) == before).all()
        # next to each other is not overlapping, and the same calls with every rule kept run
        assert dev(curve, n, d_big, None, d_b, None, 0, 0, dst=at(d_big, n * rec), total=at(d_big, 2 * n * rec)) == OK
        assert dinv(n, d_big, at(d_big, 2 * n * rec + rec), c=at(d_big, 2 * n * rec + rec - 8)) == OK
        got = d.down(d_big, (4 * n, f.limbs))
        assert (got[n:2 * n] == f.records(model.scan(f.r, n, a, b)[0], True)).all()
        assert (got[2 * n + 1:3 * n + 1] == f.records(model.invert(f.r, a)[0], True)).all()
        assert (got[3 * n + 1:] == SENTINEL).all()


# ---- end to end: device entries only between upload and download ------------------------------------------------------------
@pytest.mark.parametrize("naive", PATHS)
def test_lagrange_coefficients(engine, naive):
    """L_i(t) = (t^n - 1) / n * w^i / (t - w^i) from the powers of w, one product step and one batch inversion; then
    sum_i L_i(t) f(w^i) = f(t) for a random f of degree < n, its evaluations from the transform"""
    curve, n = 0, 1 << 10
    f = model.field(curve)
    r, w = f.r, f.root(n)
    rng = random.Random(11)
    t = rng.randrange(r)
    coeffs = [rng.randrange(r) for _ in range(n)]
    rec = f.limbs * 8
    k = (pow(t, n, r) - 1) * fr_inverse(curve, n) % r
    assert fr_inverse(curve, n) == pow(n, r - 2, r)
    with path(naive), Dev(engine) as d:
        d_w, d_t, d_den, d_inv, d_l = (d.buf(n * rec) for _ in range(5))
        d_one, d_f, d_sum = d.up(f.records([1] * n, False)), d.up(f.records(coeffs, False)), d.buf(rec)
        d_zero = d.buf(8)
        engine.fr_powers_device(curve, w, n, d_w)
        engine.fr_muladd_device(curve, n, d_one, d_one, d_t, k=t)      # every record t
        engine.fr_muladd_device(curve, n, d_t, d_one, d_den, d_c=d_w)  # t * 1 - w^i
        engine.fr_batch_invert_device(curve, n, d_den, d_inv, d_zero)
        engine.fr_muladd_device(curve, n, d_w, d_inv, d_l, k=k)        # w^i / (t - w^i) * (t^n - 1) / n
        got = f.ints(d.down(d_l, (n, f.limbs)), False)
        assert int(d.down(d_zero, (1,))[0]) == 0
        want = [k * pow(w, i, r) * pow((t - pow(w, i, r)) % r, r - 2, r) % r for i in range(n)]
        assert got == want
        # f on the domain, times L_i(t), summed by a scan of sums
        engine.fr_fft_device(curve, d_f, n, d_f)
        engine.fr_muladd_device(curve, n, d_f, d_l, d_f)
        engine.fr_scan_device(curve, n, d_f, None, d_f, d_total=d_sum)
        assert f.ints(d.down(d_sum, (1, f.limbs)), False) == [poly_eval(coeffs, t, r)]


@pytest.mark.parametrize("naive", PATHS)
def test_grand_product(engine, naive):
    """den a permutation of num: the exclusive prefix products of num_i / den_i are the z vector, and the total is 1"""
    curve, n = 1, 3000
    f = model.field(curve)
    r = f.r
    rng = random.Random(12)
    num = [rng.randrange(1, r) for _ in range(n)]
    den = list(num)
    rng.shuffle(den)
    rec = f.limbs * 8
    with path(naive), Dev(engine) as d:
        d_num, d_den, d_z, d_tot = d.up(f.records(num, False)), d.up(f.records(den, False)), d.buf(n * rec), d.buf(rec)
        engine.fr_batch_invert_device(curve, n, d_den, d_den)
        engine.fr_muladd_device(curve, n, d_num, d_den, d_z)
        engine.fr_scan_device(curve, n, d_z, d_z, exclusive=True, d_total=d_tot)
        z, tot = f.ints(d.down(d_z, (n, f.limbs)), False), f.ints(d.down(d_tot, (1, f.limbs)), False)
    ratios = [x * pow(y, r - 2, r) % r for x, y in zip(num, den)]
    want, wtot = model.scan(r, n, ratios, exclusive=True)
    assert z == want and tot == [wtot] == [1] and z[0] == 1


@pytest.mark.parametrize("naive", PATHS)
def test_kzg_quotient_into_the_msm(engine, port, naive):
    """synthetic division of a random p at a random z with total = p(z); the quotient as it lies in HBM is the scalar
    vector of an MSM over [tau^i] G, which gives [q(tau)] G"""
    curve, n = 0, 1 << 10
    f = model.field(curve)
    r = f.r
    rng = random.Random(13)
    p = [rng.randrange(r) for _ in range(n)]
    z, tau = rng.randrange(r), rng.randrange(1, r)
    grp = gmodel.group_of(port, "alt_bn128_g1")
    assert grp.r == r
    s = libff_amd.sizes(grp.curve, grp.group)
    rec = f.limbs * 8
    with path(naive), Dev(engine) as d:
        d_p, d_q, d_pz = d.up(f.records(p, False)), d.buf(n * rec), d.buf(rec)
        engine.fr_scan_device(curve, n, d_q, None, d_p, a_const=z, init=0, reverse=True, exclusive=True, d_total=d_pz)
        q, pz = f.ints(d.down(d_q, (n, f.limbs)), False), f.ints(d.down(d_pz, (1, f.limbs)), False)[0]
        assert model.synthetic_division_holds(r, p, z, q, pz) and pz == poly_eval(p, z, r)
        # the bases [tau^i] G: n copies of G times the powers of tau
        d_g, d_gaff = d.up(np.repeat(grp.records([1]), n, axis=0)), d.buf(n * s["affine_bytes"])
        d_tau, d_xyz, d_bases, d_pt = d.buf(n * rec), d.buf(n * s["g_bytes"]), d.buf(n * s["affine_bytes"]), d.buf(s["g_bytes"])
        engine.import_bases_device(grp.curve, grp.group, d_g, s["g_bytes"], multi_exp_base_form_special, n, d_gaff)
        engine.fr_powers_device(curve, tau, n, d_tau)
        engine.scalar_mul_vec_device(grp.curve, grp.group, d_gaff, d_tau, n, d_xyz, out_form=OUT_AFFINE)
        engine.import_bases_device(grp.curve, grp.group, d_xyz, s["g_bytes"], multi_exp_base_form_special, n, d_bases)
        engine.msm_device(grp.curve, grp.group, d_bases, d_q, n, d_pt, out_form=OUT_AFFINE)
        got = d.down(d_pt, (1, grp.gl))
    assert (got == grp.records([poly_eval(q, tau, r)])).all()
