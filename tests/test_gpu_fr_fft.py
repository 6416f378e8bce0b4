"""The FFT over a vector of Fr scalars on the device (Engine.fr_fft / fr_fft_device / fr_powers_device /
fr_muladd_device), all six scalar fields.  Expected values come from tests/fr_fft_model.py -- Python integers, the
definition of the transform -- and everything is compared bit for bit, as records.  Nothing here knows how a pass
walks its tile; the sizes are chosen from what libff_amd.plan_fr_fft reports: T the default tile, t the smallest."""
import ctypes
import random

import numpy as np
import pytest

import fr_fft_model as model
import group_fft_model as gmodel
from fr_dev import BAD_ARG, FOUR, OK, SENTINEL, TOO_LARGE, UNSUPPORTED, Dev, at, hip_runtime

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, fft_twiddles, multi_exp_base_form_special, plan_fr_fft  # noqa: E402

CURVES = sorted(model.CURVES)
IDS = [model.CURVES[c] for c in CURVES]
THREE = FOUR[:3]   # 8, 10, 12 words


def tiles(curve):
    p = plan_fr_fft(curve, 1)
    return p["tile_log2"], p["tile_min"]


_want = {}


def expected(curve, n, seed=0):
    """(inputs, the model's transform with libff's root) of the shared random vector: computed once"""
    key = (curve, n, seed)
    if key not in _want:
        f = model.field(curve)
        a = model.random_vector(curve, n, seed)
        _want[key] = (a, model.fft(a, f.root(n), f.r))
    return _want[key]


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_sizes(engine, curve):
    f = model.field(curve)
    T, _ = tiles(curve)
    for n in (1, 2, 4, 8, 64, 128, 256, 1 << T, 1 << (T + 1)):
        if n > 1 << f.s:
            continue
        a, want = expected(curve, n)
        for plain in (False, True):
            got = engine.fr_fft(curve, f.records(a, plain), plain=plain)
            assert got.shape == (n, f.limbs)
            assert (got == f.records(want, plain)).all(), (n, plain)
    assert engine.fr_fft(curve, np.zeros((0, f.limbs), dtype=np.uint64)).shape == (0, f.limbs)
    # n = 1 writes scale * a_0 and wants no omega
    one = engine.fr_fft(curve, f.records([5], False), scale=3)
    assert (one == f.records([15], False)).all()


@pytest.mark.parametrize("curve", THREE)
def test_pass_structure_at_the_smallest_tile(engine, curve):
    """one pass; a second pass of one stage; two full passes; three and four passes with a partial last one"""
    f = model.field(curve)
    _, t = tiles(curve)
    for lg, passes in ((t, 1), (t + 1, 2), (2 * t, 2), (2 * t + 1, 3), (3 * t + 1, 4)):
        n = 1 << lg
        assert plan_fr_fft(curve, n, t)["passes"] == passes
        a, want = expected(curve, n)
        recs = f.records(a, False)
        small = engine.fr_fft(curve, recs, tile_log2=t)
        assert (small == f.records(want, False)).all(), lg
        assert (small == engine.fr_fft(curve, recs)).all(), lg


@pytest.mark.parametrize("curve", THREE)
def test_three_passes_at_the_default_tile(engine, curve):
    f = model.field(curve)
    T, _ = tiles(curve)
    lg = min(2 * T + 1, f.s)
    n = 1 << lg
    assert plan_fr_fft(curve, n)["passes"] == 3
    w = f.root(n)
    rng = random.Random(curve + 77)
    where = sorted(rng.sample(range(n), 5))
    vals = [rng.randrange(1, f.r) for _ in where]
    recs = np.zeros((n, f.limbs), dtype=np.uint64)
    recs[where] = f.records(vals, False)
    got = engine.fr_fft(curve, recs)
    idx = sorted(set(rng.sample(range(n), 4096)) | {0, 1, n // 2, n - 1})
    want = [sum(v * pow(w, i * j % n, f.r) for i, v in zip(where, vals)) % f.r for j in idx]
    assert (got[idx] == f.records(want, False)).all()
    # a dense vector forward and back: canonical residues below 2^(bits - 1), any of which is a valid record
    dense = np.random.default_rng(curve).integers(0, 1 << 64, size=(n, f.limbs), dtype=np.uint64)
    top = f.r.bit_length() - 1 - 64 * (f.limbs - 1)
    dense[:, -1] &= np.uint64((1 << top) - 1)
    back = engine.fr_fft(curve, engine.fr_fft(curve, dense), inverse=True)
    assert (back == dense).all()


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_parameters(engine, curve):
    f = model.field(curve)
    T, _ = tiles(curve)
    n = 64
    a, w = model.random_vector(curve, n), f.root(n)
    rng = random.Random(curve + 5)
    pre, post, scale = (rng.randrange(2, f.r) for _ in range(3))
    for kw in ({"pre": pre}, {"post": post}, {"scale": scale}, {"pre": pre, "post": post, "scale": scale}):
        want = model.fft(a, w, f.r, **kw)
        for plain in (False, True):
            got = engine.fr_fft(curve, f.records(a, plain), plain=plain, **kw)
            assert (got == f.records(want, plain)).all(), (sorted(kw), plain)
    # the flags are those parameters: a coset transform, and its inverse brings the input back
    g = model.GENERATOR[curve]
    assert (engine.fr_fft(curve, f.records(a, False), coset=g) == f.records(model.fft(a, w, f.r, pre=g), False)).all()
    n = min(1 << (T + 1), 1 << f.s)
    a, _ = expected(curve, n)
    recs = f.records(a, False)
    there = engine.fr_fft(curve, recs, coset=g)
    assert (there != recs).any()
    assert (engine.fr_fft(curve, there, coset=g, inverse=True) == recs).all()


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_closed_forms(engine, curve):
    f = model.field(curve)
    T, _ = tiles(curve)
    n = min(1 << (T + 1), 1 << f.s)
    w = f.root(n)
    run = lambda vals: f.ints(engine.fr_fft(curve, f.records(vals, False)), False)
    assert run([0] * n) == [0] * n
    c = random.Random(curve).randrange(1, f.r)
    assert run([c] * n) == [n * c % f.r] + [0] * (n - 1)
    i = n // 2 + 3
    assert run([0] * i + [1] + [0] * (n - i - 1)) == [pow(w, i * j % n, f.r) for j in range(n)]
    assert run([f.r - 1] * n) == [(f.r - n) % f.r] + [0] * (n - 1)


@pytest.mark.parametrize("curve", THREE)
def test_device_entry(engine, curve):
    f = model.field(curve)
    T, _ = tiles(curve)
    rec = f.limbs * 8
    hip = hip_runtime()
    T, t = tiles(curve)
    # two passes at the default tile; three at the smallest, where an in-place call takes a second vector
    for tile, n, passes in ((0, 1 << (T + 1), 2), (t, 1 << (2 * t + 1), 3)):
        assert plan_fr_fft(curve, n, tile)["passes"] == passes
        a, want = expected(curve, n)
        want = f.records(want, False)
        with Dev(engine) as d:
            d_in = d.up(f.records(a, False))
            guard = np.full((n + 4, f.limbs), SENTINEL, dtype=np.uint64)
            d_out = d.up(guard)
            engine.fr_fft_device(curve, d_in, n, at(d_out, 2 * rec), tile_log2=tile)
            got = d.down(d_out, (n + 4, f.limbs))
            assert (got[2:-2] == want).all() and (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
            # a partial overlap is refused with nothing written
            h_in = d.down(d_in, (n, f.limbs))
            with pytest.raises(libff_amd.AmdMsmError, match="overlap"):
                engine.fr_fft_device(curve, d_in, n // 2, at(d_in, rec))
            with pytest.raises(libff_amd.AmdMsmError, match="overlap"):
                engine.fr_fft_device(curve, at(d_in, rec), n // 2, d_in)
            assert (d.down(d_in, (n, f.limbs)) == h_in).all()
            # in place, on a stream of the caller's
            stream = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
            try:
                engine.fr_fft_device(curve, d_in, n, d_in, tile_log2=tile, stream=stream)
                assert hip.hipStreamSynchronize(stream) == 0
            finally:
                assert hip.hipStreamDestroy(stream) == 0
            assert (d.down(d_in, (n, f.limbs)) == want).all()


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_a_root_that_is_no_root_is_refused(engine, curve):
    f = model.field(curve)
    n = 8
    recs = f.records(model.random_vector(curve, n), False)
    out = np.full_like(recs, SENTINEL)
    for omega in (1, f.root(16), f.root(4), 0):
        with pytest.raises(libff_amd.AmdMsmError, match="root of unity"):
            engine.fr_fft(curve, recs, omega=omega, out=out)
        assert (out == SENTINEL).all()
    with Dev(engine) as d:
        d_in, d_out = d.up(recs), d.up(out)
        for omega in (1, f.root(16)):
            with pytest.raises(libff_amd.AmdMsmError, match="root of unity"):
                engine.fr_fft_device(curve, d_in, n, d_out, omega=omega)
        assert (d.down(d_out, out.shape) == SENTINEL).all()
    # n above the 2-adicity fails the same check, whatever omega is
    if f.s < 28:
        big = np.zeros((1 << (f.s + 1), f.limbs), dtype=np.uint64)
        with pytest.raises(libff_amd.AmdMsmError, match="root of unity"):
            engine.fr_fft(curve, big, omega=f.root(1 << f.s))


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_refused_calls_name_the_condition_and_leave_the_output_alone(engine, curve):
    """both entries, with a context: the code, what amdmsm_last_error says, and the output untouched"""
    f = model.field(curve)
    n, rec = 8, f.limbs * 8
    recs = f.records(model.random_vector(curve, n), False)
    out = np.full_like(recs, SENTINEL)
    w = f.records([f.root(n)], False)
    o, bad_opts = engine._opts(), engine._opts()
    bad_opts.struct_size += 8
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: engine.lib.amdmsm_last_error(engine.h)

    def cases(call, src, dst):
        """call(curve, values, n, omega, tile, opts, out)"""
        for m in (3, 6):
            assert call(curve, src, m, ptr(w), 0, o, dst) == BAD_ARG and b"power of two" in err(), m
        assert call(curve, None, n, ptr(w), 0, o, dst) == BAD_ARG and b"values" in err()
        assert call(curve, src, n, ptr(w), 0, o, None) == BAD_ARG and b"output" in err()
        assert call(curve, src, n, None, 0, o, dst) == BAD_ARG and b"omega" in err() and b"null" in err()
        for tile in (3, 9, -1):
            assert call(curve, src, n, ptr(w), tile, o, dst) == BAD_ARG and b"tile_log2" in err(), tile
        assert call(curve, src, n, ptr(w), 0, bad_opts, dst) == BAD_ARG and b"struct_size" in err()
        assert call(curve, src, 1 << 29, ptr(w), 0, o, dst) == TOO_LARGE and b"2^28" in err()
        assert call(6, src, n, ptr(w), 0, o, dst) == UNSUPPORTED
        assert call(curve, src, n, ptr(w), 0, o, dst) == OK     # and with every rule kept the same call runs

    def host(c, src, m, omega, tile, opts, dst):
        return engine.lib.amdmsm_fr_fft(engine.h, c, src, ctypes.c_size_t(m), omega, None, None, None, tile,
                                        ctypes.byref(opts), dst)

    def dev(c, src, m, omega, tile, opts, dst):
        return engine.lib.amdmsm_fr_fft_device(engine.h, c, src, ctypes.c_size_t(m), omega, None, None, None, tile,
                                               ctypes.byref(opts), dst)

    want = f.records(model.fft(f.ints(recs, False), f.root(n), f.r), False)
    # the last call of cases() is the one that may write: everything before it is checked against the sentinels
    class Watch:
        def __init__(self, call, read):
            self.call, self.read = call, read

        def __call__(self, *args):
            rc = self.call(*args)
            if rc != OK:
                assert (self.read() == SENTINEL).all(), args[2:5]
            return rc

    cases(Watch(host, lambda: out), ptr(recs), ptr(out))
    assert (out == want).all()
    with Dev(engine) as d:
        d_in, d_out = d.up(recs), d.up(np.full_like(recs, SENTINEL))
        cases(Watch(dev, lambda: d.down(d_out, recs.shape)), d_in, d_out)
        assert (d.down(d_out, recs.shape) == want).all()
        # a device vector off its alignment (the records are moved 16 bytes at a time, 8 for the 10-word fields)
        d_big = d.up(np.full((n + 1, f.limbs), SENTINEL, dtype=np.uint64))
        assert dev(curve, d_in, n, ptr(w), 0, o, at(d_big, 4)) == BAD_ARG and b"aligned" in err()
        assert dev(curve, at(d_big, 4), n, ptr(w), 0, o, d_out) == BAD_ARG and b"aligned" in err()
        assert (d.down(d_big, (n + 1, f.limbs)) == SENTINEL).all()


@pytest.mark.parametrize("curve", THREE)
def test_twiddle_cache(engine, curve):
    f = model.field(curve)
    n, m = 512, 128
    a, want = expected(curve, n)
    b, want_b = expected(curve, m)
    recs, recs_b = f.records(a, False), f.records(b, False)
    w, ninv = f.root(n), pow(n, -1, f.r)
    fwd = f.records(want, False)
    inv = f.records(model.fft(a, pow(w, -1, f.r), f.r, scale=ninv), False)
    other = f.records(model.fft(a, pow(w, 3, f.r), f.r), False)
    assert (engine.fr_fft(curve, recs) == fwd).all()
    assert (engine.fr_fft(curve, recs, inverse=True) == inv).all()
    assert (engine.fr_fft(curve, recs) == fwd).all()
    assert (engine.fr_fft(curve, recs_b) == f.records(want_b, False)).all()
    assert (engine.fr_fft(curve, recs) == fwd).all()
    assert (engine.fr_fft(curve, recs, omega=pow(w, 3, f.r)) == other).all()   # a third root over the first domain
    assert (engine.fr_fft(curve, recs, inverse=True) == inv).all()
    assert (engine.fr_fft(curve, recs) == fwd).all()


@pytest.mark.parametrize("curve", CURVES, ids=IDS)
def test_powers(engine, curve):
    f = model.field(curve)
    base = random.Random(curve + 11).randrange(2, f.r)
    with Dev(engine) as d:
        for n in (0, 1, 2, 255, 256, 257, (1 << 16) + 1):
            guard = np.full((n + 2, f.limbs), SENTINEL, dtype=np.uint64)
            d_out = d.up(guard)
            plain = n % 2 == 0
            engine.fr_powers_device(curve, base, n, d_out, plain=plain)
            got = d.down(d_out, (n + 2, f.limbs))
            want, x = [], 1
            for _ in range(n):
                want.append(x)
                x = x * base % f.r
            assert (got[:n] == f.records(want, plain)).all(), n
            assert (got[n:] == SENTINEL).all(), n
        # the twiddles of group_fft, from their own root
        for n in (2, 64, 1 << min(17, f.s)):
            tw = fft_twiddles(curve, n)
            root = gmodel.to_int(tw[1]) if n > 2 else f.r - 1
            d_tw = d.buf(tw.nbytes)
            engine.fr_powers_device(curve, root, n // 2, d_tw, plain=True)
            assert (d.down(d_tw, tw.shape) == tw).all(), n


def test_powers_feed_group_fft(engine, port):
    """group_fft_device on twiddles made by fr_powers_device: what tests/group_fft_model.py expects"""
    name, n = "alt_bn128_g1", 64
    g = gmodel.group_of(port, name)
    tw = fft_twiddles(g.curve, n)
    w = gmodel.to_int(tw[1])
    logs = [random.Random(3).randrange(1, g.r) for _ in range(n)]
    _, pts, want = gmodel.case(port, name, logs, w)
    s = libff_amd.sizes(g.curve, g.group)
    with Dev(engine) as d:
        d_xyz, d_aff, d_tw, d_out = d.up(pts), d.buf(n * s["affine_bytes"]), d.buf(tw.nbytes), d.buf(n * s["g_bytes"])
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], multi_exp_base_form_special, n, d_aff)
        engine.fr_powers_device(g.curve, w, n // 2, d_tw)   # Montgomery records, the device entry's default
        engine.group_fft_device(g.curve, g.group, d_aff, n, d_tw, d_out, out_form=OUT_AFFINE)
        assert (d.down(d_out, (n, g.gl)) == want).all()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "mnt4_g1"])
def test_into_the_msm_without_a_host_copy(engine, port, name):
    """fr_fft_device writes the buffer msm_device reads its scalars from"""
    g = gmodel.group_of(port, name)
    f = model.field(g.curve)
    n = 256
    a, e = expected(g.curve, n)
    logs = [random.Random(9).randrange(1, g.r) for _ in range(n)]
    bases = g.records(logs)
    want = g.records([sum(x * y for x, y in zip(e, logs)) % g.r])
    s = libff_amd.sizes(g.curve, g.group)
    with Dev(engine) as d:
        d_xyz, d_aff = d.up(bases), d.buf(n * s["affine_bytes"])
        d_sc, d_out = d.up(f.records(a, False)), d.buf(s["g_bytes"])
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], multi_exp_base_form_special, n, d_aff)
        engine.fr_fft_device(g.curve, d_sc, n, d_sc)
        engine.msm_device(g.curve, g.group, d_aff, d_sc, n, d_out, out_form=OUT_AFFINE)
        assert (d.down(d_out, (1, g.gl)) == want).all()


def _poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % r
    return out


def test_quotient(engine):
    """h = (A B - C) / (x^n - 1) through the new entries only: three inverse FFTs, three coset FFTs, one muladd by
    (g^n - 1)^-1, one inverse coset FFT"""
    curve, n = 3, 64
    f = model.field(curve)
    r, g, w = f.r, model.GENERATOR[curve], f.root(n)
    a, b = model.random_vector(curve, n, 1), model.random_vector(curve, n, 2)
    c = [x * y % r for x, y in zip(a, b)]
    k = pow(pow(g, n, r) - 1, -1, r)
    with Dev(engine) as d:
        bufs = [d.up(f.records(v, False)) for v in (a, b, c)]
        for p in bufs:
            engine.fr_fft_device(curve, p, n, p, inverse=True)
            engine.fr_fft_device(curve, p, n, p, coset=g)
        d_h = d.buf(n * f.limbs * 8)
        engine.fr_muladd_device(curve, n, bufs[0], bufs[1], d_h, d_c=bufs[2], k=k)
        engine.fr_fft_device(curve, d_h, n, d_h, coset=g, inverse=True)
        h = f.ints(d.down(d_h, (n, f.limbs)), False)
        # the step alone, plain records, no c, no k
        engine.fr_muladd_device(curve, n, d.up(f.records(a, True)), d.up(f.records(b, True)), d_h, plain=True)
        assert f.ints(d.down(d_h, (n, f.limbs)), True) == c
    winv, ninv = pow(w, -1, r), pow(n, -1, r)
    A, B, C = (model.fft(v, winv, r, scale=ninv) for v in (a, b, c))
    lhs = _poly_mul(A, B, r)
    for i, x in enumerate(C):
        lhs[i] = (lhs[i] - x) % r
    rhs = [0] * (2 * n - 1)
    for i, x in enumerate(h[:n - 1]):   # h (x^n - 1)
        rhs[i + n] = (rhs[i + n] + x) % r
        rhs[i] = (rhs[i] - x) % r
    assert h[n - 1] == 0
    assert lhs == rhs
