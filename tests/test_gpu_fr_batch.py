"""Batched transforms over Fr on the device (Engine.fr_fft_batch / fr_fft_batch_device / fr_domain_fft_batch_device): every
vector of a batch against the definition in tests/fr_fft_model.py and, bit for bit, against one single-vector call per
vector.  The shapes are the smallest at which the batched pass can go wrong: fewer records than a workgroup's tile of
2^10 (several vectors in one workgroup, a last workgroup that is short of vectors), exactly 2^10, several tiles per
vector, one, two and three passes, in place with the second workspace set, strides with sentinels in the gaps."""
import ctypes

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm
from fr_dev import BAD_ARG, SENTINEL, TOO_LARGE, Dev, at, hip_runtime

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402

SIX = [pytest.param(c, id=n) for c, n in fm.CURVES.items()]
THREE = [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4"), pytest.param(2, id="bw6_761")]
_expected = {}


def vectors(curve, n, batch):
    return [fm.random_vector(curve, n, seed=100 + v) for v in range(batch)]


def expected(curve, n, batch):
    """the batch's vectors and their transforms with libff's root, computed once"""
    key = (curve, n, batch)
    if key not in _expected:
        f = fm.field(curve)
        a = vectors(curve, n, batch)
        w = f.root(n) if n > 1 else 1
        _expected[key] = (a, [(fm.naive if n <= 64 else fm.fft)(v, w, f.r) for v in a])
    return _expected[key]


def packed(f, vecs, plain):
    n = len(vecs[0])
    return np.stack([f.records(v, plain) for v in vecs]) if n else np.zeros((len(vecs), 0, f.limbs), dtype=np.uint64)


@pytest.mark.parametrize("curve", SIX)
def test_small_sizes_on_every_field_in_both_record_forms(engine, curve):
    """n = 64 with 17 vectors: 16 vectors to a workgroup, one full workgroup and one that holds a single vector"""
    f = fm.field(curve)
    for n in (1, 2, 8, 64):
        for batch in (1, 3, 17):
            a, want = expected(curve, n, batch)
            p = libff_amd.plan_fr_fft_batch(curve, n, batch)
            assert p["vectors_per_workgroup"] == 1024 // n and p["workgroups"] == (batch * n + 1023) // 1024
            for plain in (False, True):
                got = engine.fr_fft_batch(curve, packed(f, a, plain), plain=plain)
                assert [f.ints(g, plain) for g in got] == want, (curve, n, batch, plain)


SHAPES = [pytest.param(1 << 8, 5, 0, False, id="256x5_V4_short_last_workgroup"),
          pytest.param(1 << 9, 3, 8, False, id="512x3_tile8_two_passes_V2"),
          pytest.param(1 << 10, 3, 0, False, id="1024x3"),
          pytest.param(1 << 12, 3, 4, True, id="4096x3_tile4_in_place_three_passes"),
          pytest.param(1 << 12, 3, 8, False, id="4096x3_tile8_out_of_place")]


@pytest.mark.parametrize("curve", THREE)
@pytest.mark.parametrize("n,batch,tile,in_place", SHAPES)
def test_against_single_calls_and_the_model(engine, curve, n, batch, tile, in_place):
    f = fm.field(curve)
    rec = f.limbs * 8
    a, want = expected(curve, n, batch)
    p = libff_amd.plan_fr_fft_batch(curve, n, batch, tile)
    assert p["passes"] == {(1 << 8, 0): 1, (1 << 9, 8): 2, (1 << 10, 0): 2, (1 << 12, 4): 3, (1 << 12, 8): 2}[(n, tile)]
    for plain in (False, True):
        recs = packed(f, a, plain)
        with Dev(engine) as d:
            d_in = d.up(recs)
            d_out = d_in if in_place else d.buf(recs.nbytes)
            d_one = d.buf(recs.nbytes)
            for v in range(batch):   # the single-vector entry, vector by vector, out of place
                engine.fr_fft_device(curve, at(d_in, v * n * rec), n, at(d_one, v * n * rec), plain=plain, tile_log2=tile)
            single = d.down(d_one, recs.shape)
            engine.fr_fft_batch_device(curve, d_in, n, batch, d_out, plain=plain, tile_log2=tile)
            got = d.down(d_out, recs.shape)
            assert (got == single).all(), (curve, n, batch, plain)
            assert [f.ints(g, plain) for g in got] == want, (curve, n, batch, plain)
            if not in_place:
                assert (d.down(d_in, recs.shape) == recs).all()


@pytest.mark.parametrize("curve", THREE)
@pytest.mark.parametrize("n,batch,tile", [(64, 17, 0), (1 << 9, 3, 4), (1 << 11, 3, 0)])
def test_strides_and_sentinels(engine, curve, n, batch, tile):
    """in_stride = n + 3, out_stride = n + 5: every gap and the records behind the last vector keep their sentinel, and
    the source keeps its records"""
    f = fm.field(curve)
    rec = f.limbs * 8
    a, want = expected(curve, n, batch)
    si, so = n + 3, n + 5
    src = np.full((batch * si + 2, f.limbs), SENTINEL, dtype=np.uint64)
    for v in range(batch):
        src[v * si:v * si + n] = f.records(a[v], False)
    dst = np.full((batch * so + 2, f.limbs), SENTINEL, dtype=np.uint64)
    with Dev(engine) as d:
        d_src, d_dst = d.up(src), d.up(dst)
        engine.fr_fft_batch_device(curve, d_src, n, batch, d_dst, in_stride=si, out_stride=so, tile_log2=tile)
        got = d.down(d_dst, dst.shape)
        for v in range(batch):
            assert f.ints(got[v * so:v * so + n], False) == want[v], (curve, n, v)
            assert (got[v * so + n:(v + 1) * so] == SENTINEL).all(), (curve, n, v)
        assert (got[batch * so:] == SENTINEL).all()
        assert (d.down(d_src, src.shape) == src).all()
        # in place with a stride, sentinels in the gaps of the one vector
        engine.fr_fft_batch_device(curve, d_src, n, batch, d_src, in_stride=si, out_stride=si, tile_log2=tile)
        got = d.down(d_src, src.shape)
        for v in range(batch):
            assert f.ints(got[v * si:v * si + n], False) == want[v], (curve, n, v)
            assert (got[v * si + n:(v + 1) * si] == SENTINEL).all(), (curve, n, v)
        assert (got[batch * si:] == SENTINEL).all()


def test_in_place_on_a_stream_of_the_callers(engine):
    curve, n, batch = 0, 1 << 11, 3
    f = fm.field(curve)
    a, want = expected(curve, n, batch)
    recs = packed(f, a, False)
    hip = hip_runtime()
    with Dev(engine) as d:
        d_buf = d.up(recs)
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        try:
            engine.fr_fft_batch_device(curve, d_buf, n, batch, d_buf, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
            got = d.down(d_buf, recs.shape)
            assert [f.ints(g, False) for g in got] == want
            engine.fr_fft_batch_device(curve, d_buf, n, batch, d_buf, inverse=True, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
        finally:
            assert hip.hipStreamDestroy(stream) == 0
        assert (d.down(d_buf, recs.shape) == recs).all()


@pytest.mark.parametrize("curve", THREE)
@pytest.mark.parametrize("n,batch,tile", [(32, 5, 0), (1 << 9, 3, 4), (1 << 12, 3, 8)])
def test_inverse_coset_form(engine, curve, n, batch, tile):
    """pre on the way there; post and scale together on the way back; there and back is the input"""
    f = fm.field(curve)
    g = fm.GENERATOR[curve]
    a = vectors(curve, n, batch)
    for plain in (False, True):
        recs = packed(f, a, plain)
        there = engine.fr_fft_batch(curve, recs, coset=g, plain=plain, tile_log2=tile)
        want = [fm.fft(v, f.root(n), f.r, pre=g) for v in a]
        assert [f.ints(t, plain) for t in there] == want, (curve, n, plain)
        back = engine.fr_fft_batch(curve, there, inverse=True, coset=g, plain=plain, tile_log2=tile)
        assert (back == recs).all(), (curve, n, plain)
        for v in range(batch):
            assert (engine.fr_fft(curve, there[v], inverse=True, coset=g, plain=plain, tile_log2=tile) == recs[v]).all()
        # the general form, all three at once
        got = engine.fr_fft_batch(curve, recs, plain=plain, tile_log2=tile, pre=g, post=3, scale=5)
        assert [f.ints(t, plain) for t in got] == [fm.fft(v, f.root(n), f.r, pre=g, post=3, scale=5) for v in a], (curve, n, plain)


@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(1, id="bls12_377")])
def test_one_shape_past_the_small_ones(engine, curve):
    """2^17 x 2 at the default tile: 256 workgroups a pass, against the single calls"""
    n, batch = 1 << 17, 2
    f = fm.field(curve)
    rec = f.limbs * 8
    recs = np.random.default_rng(17 + curve).integers(0, 1 << 60, size=(batch, n, f.limbs), dtype=np.uint64)   # below 2^252 < r
    assert libff_amd.plan_fr_fft_batch(curve, n, batch)["workgroups"] == 256
    with Dev(engine) as d:
        d_in, d_out, d_one = d.up(recs), d.buf(recs.nbytes), d.buf(recs.nbytes)
        for v in range(batch):
            engine.fr_fft_device(curve, at(d_in, v * n * rec), n, at(d_one, v * n * rec))
        engine.fr_fft_batch_device(curve, d_in, n, batch, d_out)
        got = d.down(d_out, recs.shape)
        assert (got == d.down(d_one, recs.shape)).all() and (got != recs).any()
        engine.fr_fft_batch_device(curve, d_out, n, batch, d_out, inverse=True)
        assert (d.down(d_out, recs.shape) == recs).all()


def test_refusals_with_a_context(engine):
    curve, n, batch = 0, 8, 3
    f = fm.field(curve)
    rec = f.limbs * 8
    err = lambda: engine.lib.amdmsm_last_error(engine.h).decode()
    a, _ = expected(curve, n, batch)
    src = packed(f, a, False)
    with Dev(engine) as d:
        d_src = d.up(src)
        d_dst = d.up(np.full((4 * batch * n, f.limbs), SENTINEL, dtype=np.uint64))
        dev = lambda **kw: engine.fr_fft_batch_device(curve, kw.pop("src", d_src), kw.pop("n", n), kw.pop("batch", batch),
                                                      kw.pop("dst", d_dst), **kw)
        cases = [
            (dict(n=6, omega=f.root(8)), BAD_ARG, "power of two"), (dict(tile_log2=9), BAD_ARG, "tile_log2"), (dict(omega=f.root(4)), BAD_ARG, "omega"),
            (dict(src=None), BAD_ARG, "values"), (dict(dst=None), BAD_ARG, "output"),
            (dict(n=1 << 20, batch=257), TOO_LARGE, "batch"), (dict(in_stride=1 << 62), TOO_LARGE, "in_stride"),
            (dict(in_stride=n - 1), BAD_ARG, "in_stride = 7 < n = 8"), (dict(out_stride=n - 1), BAD_ARG, "out_stride = 7 < n = 8"),
            (dict(src=at(d_src, 4)), BAD_ARG, "aligned"), (dict(dst=at(d_dst, 4)), BAD_ARG, "aligned"),
            (dict(dst=at(d_src, rec)), BAD_ARG, "overlap"), (dict(src=at(d_dst, rec)), BAD_ARG, "overlap"),
            (dict(dst=d_src, out_stride=n + 1), BAD_ARG, "overlap"),
        ]
        for kw, code, words in cases:
            with pytest.raises(libff_amd.AmdMsmError) as e:
                dev(**kw)
            assert e.value.code == code and words in err(), (kw, err())
        with pytest.raises(libff_amd.AmdMsmError, match="domain size") as e:
            engine.fr_domain_fft_batch_device(curve, d_src, 7, batch, d_dst)
        assert e.value.code == BAD_ARG
        with pytest.raises(libff_amd.AmdMsmError, match="in_stride = 5 < m = 6") as e:
            engine.fr_domain_fft_batch_device(curve, d_src, 6, batch, d_dst, in_stride=5)
        assert e.value.code == BAD_ARG
        assert (d.down(d_dst, (4 * batch * n, f.limbs)) == SENTINEL).all()
        assert (d.down(d_src, src.shape) == src).all()
        # batch = 0 and n = 0 succeed and write nothing, null vectors included
        engine.fr_fft_batch_device(curve, d_src, n, 0, d_dst)
        engine.fr_fft_batch_device(curve, None, n, 0, None)
        engine.fr_fft_batch_device(curve, None, 0, batch, None)
        engine.fr_domain_fft_batch_device(curve, None, 6, 0, None)
        assert (d.down(d_dst, (4 * batch * n, f.limbs)) == SENTINEL).all()
        assert engine.fr_fft_batch(curve, np.zeros((0, n, f.limbs), dtype=np.uint64)).shape == (0, n, f.limbs)
        assert engine.fr_fft_batch(curve, np.zeros((batch, 0, f.limbs), dtype=np.uint64)).shape == (batch, 0, f.limbs)
        # and the context serves the next call
        engine.fr_fft_batch_device(curve, d_src, n, batch, d_dst)
        assert (d.down(d_dst, src.shape) != SENTINEL).any()


DOMAINS = [3, 6, 24, (1 << 10) + (1 << 4)]


@pytest.mark.parametrize("curve", [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4")])
@pytest.mark.parametrize("m", DOMAINS)
def test_domain_batch(engine, curve, m):
    """three vectors over a step domain, forward and inverse, with and without the coset: the model for the small sizes,
    the single-vector entry for all; strided, with sentinels in the gaps"""
    f = fm.field(curve)
    rec = f.limbs * 8
    batch, stride = 3, m + 2
    a = vectors(curve, m, batch)
    for plain in (False, True):
        for g in (None, fm.GENERATOR[curve]):
            for inverse in (False, True):
                buf = np.full((batch * stride, f.limbs), SENTINEL, dtype=np.uint64)
                for v in range(batch):
                    buf[v * stride:v * stride + m] = f.records(a[v], plain)
                with Dev(engine) as d:
                    d_in, d_out, d_one = d.up(buf), d.up(np.full_like(buf, SENTINEL)), d.up(np.full_like(buf, SENTINEL))
                    for v in range(batch):
                        engine.fr_domain_fft_device(curve, at(d_in, v * stride * rec), m, at(d_one, v * stride * rec), inverse=inverse,
                                                    coset=g, plain=plain)
                    single = d.down(d_one, buf.shape)
                    engine.fr_domain_fft_batch_device(curve, d_in, m, batch, d_out, in_stride=stride, out_stride=stride,
                                                      inverse=inverse, coset=g, plain=plain)
                    got = d.down(d_out, buf.shape)
                    assert (got == single).all(), (curve, m, plain, g, inverse)
                    assert (d.down(d_in, buf.shape) == buf).all()
                    engine.fr_domain_fft_batch_device(curve, d_in, m, batch, d_in, in_stride=stride, out_stride=stride,
                                                      inverse=inverse, coset=g, plain=plain)
                    assert (d.down(d_in, buf.shape) == single).all(), (curve, m, plain, g, inverse, "in place")
                if m <= 24:
                    fn = dm.interpolate if inverse else dm.transform
                    for v in range(batch):
                        assert f.ints(got[v * stride:v * stride + m], plain) == fn(curve, a[v], g or 1), (curve, m, v, plain, g, inverse)
