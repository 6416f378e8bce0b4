"""Radix-2 FFT over a point vector, out[j] = sum_i w^(i j) P_i (Engine.group_fft / group_fft_device), all eleven groups.
Expected values come from tests/group_fft_model.py: every input is a known multiple of the generator, every expected
output the generator times sum_i w^(i j) a_i mod r.  Everything is compared as special-form records, bit for bit.  Nothing
here knows the order of the stages or the window width of the ladder.

bw6_761 (a lone ladder of its 24-word field takes about 45 ms) stays at n <= 64."""
import ctypes
import random

import numpy as np
import pytest

import group_fft_model as model

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G2, MNT6, OUT_AFFINE, OUT_LIBFF, fft_twiddles, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special)

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
ALL = [pytest.param(n, id=n) for n in model.ALL_NAMES]
SPECIAL, NORMAL = multi_exp_base_form_special, multi_exp_base_form_normal
SENTINEL = 0x5a5a5a5a5a5a5a5a
# 2: no ladder; 4: the first laddered stage; 8: the smallest size whose index permutation is not an involution of
# neighbours; 128: exactly one wave of butterflies; 256: two waves
SIZES = [1, 2, 4, 8, 64, 128, 256]


def sizes_of(name):
    return [n for n in SIZES if n <= 64 or not name.startswith("bw6_761")]


def root(g, n, inverse=False):
    """the root whose powers fft_twiddles returns, as an integer"""
    if n < 2:
        return 1
    if n == 2:
        return g.r - 1
    return model.to_int(fft_twiddles(g.curve, n, inverse=inverse)[1])


def twiddles(g, n, plain, inverse=False):
    tw = fft_twiddles(g.curve, n, inverse=inverse)
    return tw if plain or not len(tw) else g.mont([model.to_int(t) for t in tw])


def random_logs(g, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, g.r) for _ in range(n)]


def run(engine, g, pts, tw, **kw):
    """the host entry, result in special form whatever the output form"""
    out_form = kw.get("out_form", OUT_LIBFF)
    got = engine.group_fft(g.curve, g.group, pts, tw, **kw)
    return got if out_form == OUT_AFFINE or len(got) == 0 else g.special(got)


def random_case(port, name, n):
    g = model.group_of(port, name)
    return model.case(port, name, random_logs(g, n, sum(name.encode()) + n), root(g, n))


@pytest.mark.parametrize("name", ALL)
def test_sizes(engine, port, name):
    for n in sizes_of(name):
        g, pts, want = random_case(port, name, n)
        got = run(engine, g, pts, twiddles(g, n, plain=True), base_form=SPECIAL, out_form=OUT_AFFINE, scalars_plain=True)
        assert got.shape == (n, g.gl)
        assert (got == want).all(), n


@pytest.mark.parametrize("name", ALL)
def test_null_twiddles_up_to_two_points_and_no_points(engine, port, name):
    g = model.group_of(port, name)
    for n in (1, 2):
        _, pts, want = random_case(port, name, n)
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            assert (run(engine, g, pts, None, base_form=SPECIAL, out_form=out_form) == want).all(), (n, out_form)
    # n = 1 of a point with Z != 1 and of infinity: the point, in special form
    _, pts, want = model.case(port, name, [5, 0], 1)
    for i in (0, 1):
        src = g.scale(pts[i:i + 1], seed=3)
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            assert (run(engine, g, src, None, base_form=NORMAL, out_form=out_form) == pts[i:i + 1]).all()
    assert engine.group_fft(g.curve, g.group, np.zeros((0, g.gl), dtype=np.uint64), None).shape == (0, g.gl)
    o = engine._opts()
    z = ctypes.c_size_t(0)
    assert engine.lib.amdmsm_group_fft(engine.h, g.curve, g.group, None, z, SPECIAL, z, None, None, z, ctypes.byref(o)) == OK
    assert engine.lib.amdmsm_group_fft_device(engine.h, g.curve, g.group, None, z, None, None, z, ctypes.byref(o)) == OK


@pytest.mark.parametrize("name", ALL)
def test_base_forms_output_forms_and_twiddle_forms(engine, port, name):
    n = 8 if name.startswith("bw6_761") else 64
    g, special, want = random_case(port, name, n)
    normal = g.scale(special, seed=11)
    assert (normal != special).any()
    for base_form, pts in ((SPECIAL, special), (NORMAL, normal)):
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            for plain in (False, True):
                got = run(engine, g, pts, twiddles(g, n, plain), base_form=base_form, out_form=out_form, scalars_plain=plain)
                assert (got == want).all(), (base_form, out_form, plain)


def device_fft(engine, g, pts, tw, n, guard_records=0, **kw):
    """the device entry on special-form records `pts`; returns the output records and the guard records behind them"""
    s = libff_amd.sizes(g.curve, g.group)
    d_xyz, d_aff = engine.malloc(n * s["g_bytes"]), engine.malloc(n * s["affine_bytes"])
    d_tw, d_out = engine.malloc(max(tw.nbytes, 8)), engine.malloc((n + guard_records) * s["g_bytes"])
    try:
        engine.h2d(d_xyz, pts)
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], SPECIAL, n, d_aff)
        if tw.nbytes:
            engine.h2d(d_tw, tw)
        out = np.full((n + guard_records, g.gl), SENTINEL, dtype=np.uint64)
        engine.h2d(d_out, out)
        engine.group_fft_device(g.curve, g.group, d_aff, n, d_tw, d_out, **kw)
        engine.synchronize()
        engine.d2h(out, d_out)
        return out[:n], out[n:]
    finally:
        for p in (d_xyz, d_aff, d_tw, d_out):
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_device_entry(engine, port, name):
    n = 8 if name.startswith("bw6_761") else 64
    g, pts, want = random_case(port, name, n)
    for out_form, plain, chunk in ((OUT_AFFINE, True, 0), (OUT_LIBFF, False, 3)):
        got, guard = device_fft(engine, g, pts, twiddles(g, n, plain), n, guard_records=2, out_form=out_form,
                                scalars_plain=plain, chunk_points=chunk)
        assert ((got if out_form == OUT_AFFINE else g.special(got)) == want).all(), (out_form, plain, chunk)
        assert (guard == SENTINEL).all()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_381_g2", "mnt4_g1"])
def test_chunks_equal_the_unchunked_call(engine, port, name):
    """n = 1024 in chunks of 192, 192 and 128 butterflies, on 1024 different points made on the device"""
    g = model.group_of(port, name)
    n = 1024
    s = libff_amd.sizes(g.curve, g.group)
    assert libff_amd.plan_group_fft(g.curve, g.group, n, chunk_points=192)["chunk_points"] == 192
    tw = twiddles(g, n, plain=True)
    d_aff, d_tw, d_out = engine.malloc(n * s["affine_bytes"]), engine.malloc(tw.nbytes), engine.malloc(n * s["g_bytes"])
    try:
        engine.gen_bases_seq_device(g.curve, g.group, 2, n, d_aff)
        engine.h2d(d_tw, tw)
        outs = []
        for chunk in (0, 192):
            engine.group_fft_device(g.curve, g.group, d_aff, n, d_tw, d_out, out_form=OUT_AFFINE, scalars_plain=True,
                                    chunk_points=chunk)
            engine.synchronize()
            got = np.zeros((n, g.gl), dtype=np.uint64)
            engine.d2h(got, d_out)
            outs.append(got)
        assert (outs[0] == outs[1]).all()
        # the inputs are 3 G, 4 G, ...: output 0 is their sum
        assert (outs[0][0] == g.records([sum(range(3, 3 + n))])[0]).all()
        assert len({row.tobytes() for row in outs[0]}) == n
    finally:
        for p in (d_aff, d_tw, d_out):
            engine.free(p)


def degenerate_logs(g, n, seed):
    rng = random.Random(seed)
    a = rng.randrange(1, g.r)
    holes = [0 if rng.random() < 0.4 else rng.randrange(1, g.r) for _ in range(n)]
    holes[rng.randrange(n)] = 0
    return {
        "all equal": [a] * n,                                       # out[0] = n P, the rest infinity
        "alternating signs": [a if i % 2 == 0 else g.r - a for i in range(n)],   # out[n/2] = n P, the rest infinity
        "impulse at 0": [a] + [0] * (n - 1),                        # every output is P: T is infinite throughout
        "impulse at 1": [0, a] + [0] * (n - 2),                     # out[j] = w^j P: the twiddle order
        "infinities at random places": holes,
    }


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("n", [8, 64])
def test_degenerate_operands(engine, port, name, n):
    g = model.group_of(port, name)
    w = root(g, n)
    for what, logs in degenerate_logs(g, n, 7 * n + sum(name.encode())).items():
        _, pts, want = model.case(port, name, logs, w)
        inf = g.records([0])[0]
        zeros = [(row == inf).all() for row in want]
        if what == "all equal":
            assert zeros == [False] + [True] * (n - 1) and (want[0] == g.records([n * logs[0]])[0]).all()
        elif what == "alternating signs":
            assert zeros == [j != n // 2 for j in range(n)] and (want[n // 2] == g.records([n * logs[0]])[0]).all()
        elif what == "impulse at 0":
            assert (want == pts[0]).all()
        elif what == "impulse at 1":
            assert (want == g.records([pow(w, j, g.r) * logs[1] for j in range(n)])).all()
        got = run(engine, g, pts, twiddles(g, n, plain=False), base_form=SPECIAL, out_form=OUT_AFFINE)
        assert (got == want).all(), what


@pytest.mark.parametrize("name", ALL)
def test_last_butterfly_meets_equal_and_opposite_operands(engine, port, name):
    """n = 4 with a_0 = a_2 + w (a_1 - a_3): the last butterfly of output 1 and 3 has A = a_0 - a_2 and T = w (a_1 - a_3)
    equal, in a decimation-in-time and in a decimation-in-frequency network alike -- one output doubles (with the a != 0
    term of the MNT curves), the other is infinity"""
    g = model.group_of(port, name)
    w = root(g, 4)
    rng = random.Random(sum(name.encode()))
    a1, a2, a3 = (rng.randrange(1, g.r) for _ in range(3))
    logs = [(a2 + w * (a1 - a3)) % g.r, a1, a2, a3]
    _, pts, want = model.case(port, name, logs, w)
    inf = g.records([0])[0]
    assert (want[3] == inf).all() and (want[1] == g.records([2 * (logs[0] - a2)])[0]).all()
    assert not (want[0] == inf).all() and not (want[2] == inf).all()
    for base_form, src in ((SPECIAL, pts), (NORMAL, g.scale(pts, seed=5))):
        for out_form in (OUT_AFFINE, OUT_LIBFF):
            got = run(engine, g, src, twiddles(g, 4, plain=False), base_form=base_form, out_form=out_form)
            assert (got == want).all(), (base_form, out_form)


@pytest.mark.parametrize("name", ALL)
def test_round_trip_on_the_device(engine, port, name):
    """forward with OUT_AFFINE, import_bases_device(form special), inverse twiddles, import again, fold by n^-1: the input"""
    n = 8 if name.startswith("bw6_761") else 64
    g, pts, _ = random_case(port, name, n)
    s = libff_amd.sizes(g.curve, g.group)
    fwd, inv = twiddles(g, n, plain=True), twiddles(g, n, plain=True, inverse=True)
    assert root(g, n) * root(g, n, inverse=True) % g.r == 1
    d_xyz, d_aff = engine.malloc(n * s["g_bytes"]), engine.malloc(n * s["affine_bytes"])
    d_fwd, d_inv = engine.malloc(fwd.nbytes), engine.malloc(inv.nbytes)
    try:
        engine.h2d(d_xyz, pts)
        engine.h2d(d_fwd, fwd)
        engine.h2d(d_inv, inv)
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], SPECIAL, n, d_aff)
        engine.group_fft_device(g.curve, g.group, d_aff, n, d_fwd, d_xyz, out_form=OUT_AFFINE, scalars_plain=True)
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], SPECIAL, n, d_aff)
        engine.group_fft_device(g.curve, g.group, d_aff, n, d_inv, d_xyz, out_form=OUT_AFFINE, scalars_plain=True)
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], SPECIAL, n, d_aff)
        engine.fold_vec_device(g.curve, g.group, [d_aff], g.mont([pow(n, -1, g.r)]), n, d_xyz, out_form=OUT_AFFINE)
        engine.synchronize()
        got = np.zeros((n, g.gl), dtype=np.uint64)
        engine.d2h(got, d_xyz)
        assert (got == pts).all()
    finally:
        for p in (d_xyz, d_aff, d_fwd, d_inv):
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_refused_calls_leave_the_output_alone(engine, port, name):
    n = 8
    g, pts, want = random_case(port, name, n)
    s = libff_amd.sizes(g.curve, g.group)
    tw = twiddles(g, n, plain=False)
    out = np.full((n, g.gl), SENTINEL, dtype=np.uint64)
    o = engine._opts(out_form=OUT_AFFINE)
    bad_opts = engine._opts(out_form=OUT_AFFINE)
    bad_opts.struct_size += 8
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: engine.lib.amdmsm_last_error(engine.h)

    def host(curve, group, src, stride, m, twd, dst, opts=o):
        return engine.lib.amdmsm_group_fft(engine.h, curve, group, src, ctypes.c_size_t(stride), SPECIAL, ctypes.c_size_t(m),
                                           twd, dst, ctypes.c_size_t(0), ctypes.byref(opts))

    for m in (3, 5, 6, 7):
        assert host(g.curve, g.group, ptr(pts), s["g_bytes"], m, ptr(tw), ptr(out)) == BAD_ARG
        assert b"power of two" in err()
    assert host(g.curve, g.group, None, s["g_bytes"], n, ptr(tw), ptr(out)) == BAD_ARG and b"points" in err()
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"], n, None, ptr(out)) == BAD_ARG and b"twiddles" in err()
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"], 4, None, ptr(out)) == BAD_ARG
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"], n, ptr(tw), None) == BAD_ARG and b"output" in err()
    # a stride that is no multiple of the record alignment (4 bytes more than a record), one shorter than a record
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"] + 4, n, ptr(tw), ptr(out)) == BAD_ARG and b"stride" in err()
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"] - 16, n, ptr(tw), ptr(out)) == BAD_ARG
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"], n, ptr(tw), ptr(out), bad_opts) == BAD_ARG and b"struct_size" in err()
    assert host(g.curve, g.group, ptr(pts), s["g_bytes"], 1 << 29, ptr(tw), ptr(out)) == TOO_LARGE
    assert host(MNT6, G2, ptr(pts), s["g_bytes"], n, ptr(tw), ptr(out)) == UNSUPPORTED
    assert (out == SENTINEL).all()

    d_aff, d_tw, d_out = engine.malloc(n * s["affine_bytes"]), engine.malloc(tw.nbytes), engine.malloc(n * s["g_bytes"])
    try:
        engine.h2d(d_out, out)
        engine.h2d(d_tw, tw)
        engine.gen_bases_seq_device(g.curve, g.group, 0, n, d_aff)

        def dev(curve, group, src, m, twd, dst, opts=o):
            return engine.lib.amdmsm_group_fft_device(engine.h, curve, group, src, ctypes.c_size_t(m), twd, dst,
                                                      ctypes.c_size_t(0), ctypes.byref(opts))

        for m in (3, 6):
            assert dev(g.curve, g.group, d_aff, m, d_tw, d_out) == BAD_ARG
        assert dev(g.curve, g.group, None, n, d_tw, d_out) == BAD_ARG
        assert dev(g.curve, g.group, d_aff, n, None, d_out) == BAD_ARG
        assert dev(g.curve, g.group, d_aff, 4, None, d_out) == BAD_ARG
        assert dev(g.curve, g.group, d_aff, n, d_tw, None) == BAD_ARG
        assert dev(g.curve, g.group, d_aff, n, d_tw, d_out, bad_opts) == BAD_ARG
        assert dev(g.curve, g.group, d_aff, 1 << 29, d_tw, d_out) == TOO_LARGE
        assert dev(MNT6, G2, d_aff, n, d_tw, d_out) == UNSUPPORTED
        engine.synchronize()
        back = np.zeros_like(out)
        engine.d2h(back, d_out)
        assert (back == SENTINEL).all()
    finally:
        for p in (d_aff, d_tw, d_out):
            engine.free(p)
    # a padded stride that keeps the alignment is accepted
    padded = np.concatenate([pts, pts], axis=1)
    got = engine.group_fft(g.curve, g.group, padded, tw, base_form=SPECIAL, out_form=OUT_AFFINE, stride_bytes=2 * s["g_bytes"])
    assert (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_twiddles_that_are_no_roots_of_unity_stay_inside_the_output(engine, port, name):
    """random Fr values, and as plain integers values up to the all-ones one: the call succeeds and writes the n output
    records and nothing behind them.  No value is checked."""
    n = 8 if name.startswith("bw6_761") else 64
    g, pts, _ = random_case(port, name, n)
    rng = random.Random(n + sum(name.encode()))
    for plain in (False, True):
        ks = [rng.randrange(g.r) for _ in range(n // 2)]
        if plain:
            ks[0], ks[1] = (1 << (64 * g.fl)) - 1, g.r
        tw = g.plain(ks) if plain else g.mont(ks)
        got, guard = device_fft(engine, g, pts, tw, n, guard_records=4, out_form=OUT_LIBFF, scalars_plain=plain)
        assert (guard == SENTINEL).all()
        assert not (got == SENTINEL).all(axis=1).any()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "mnt4_g2"])
def test_timings_add_up(engine, port, name):
    """with timing enabled the phases of all stages are summed: they add up to the call"""
    n = 64
    g, pts, want = random_case(port, name, n)
    engine.set_timing(True)
    try:
        got = run(engine, g, pts, twiddles(g, n, plain=True), base_form=SPECIAL, out_form=OUT_AFFINE, scalars_plain=True)
        ms = (ctypes.c_float * libff_amd.engine.MAX_PHASES)()
        assert engine.lib.amdmsm_get_timings(engine.h, ms) == OK
    finally:
        engine.set_timing(False)
    assert (got == want).all()
    total = ms[libff_amd.engine.PH_TOTAL]
    assert total > 0 and all(ms[i] > 0 for i in range(4)) and ms[4] == 0
    assert abs(sum(ms[i] for i in range(4)) - total) <= 0.02 * total + 0.01
    assert ms[2] > ms[1]   # five ladders of 65 windows against five tables of 8 entries
