"""amdmsm_batch_exp_device: batch_exp on device-resident scalars with the results left in HBM, all eleven groups -- table
shapes and batch sizes at the edges of the 256-lane workgroup, Montgomery and plain scalars, coefficients 0, 1, r - 1, the
three output forms, the resident table shared with the host entry in both directions and across streams, sentinels
around the output, every refusal with its message, n = 0, and a powers-of-tau SRS from t to a file the stream reader
takes.

No expectation comes from the device: every element is compared, as an affine point, with the closed form of
tests/fixed_base_cases.py; the SRS with (sum s_i t^i mod r) G from Python integers."""
import ctypes
import random

import numpy as np
import pytest

import fixed_base_cases as fb
from fr_dev import hip_runtime

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, OUT_JACOBIAN, OUT_LIBFF  # noqa: E402

BAD_ARG, UNSUPPORTED = -2, -3
SENTINEL = 0xA5A5A5A5A5A5A5A5
PAD = 64   # words of sentinel on either side of the output
_groups, _expect = {}, {}


def _grp(port, name):
    if name not in _groups:
        _groups[name] = fb.group_of(port, name)
    return _groups[name]


class Expect:
    """closed-form affine keys of k g for one base, one scalar multiplication per distinct multiplier, kept"""

    def __init__(self, grp, g):
        self.grp, self.g, self.memo = grp, g, {}

    def keys(self, ks, coeff=None):
        grp = self.grp
        if coeff is not None:
            ks = [coeff * k % grp.r for k in ks]
        new = [k for k in dict.fromkeys(ks) if k not in self.memo]
        for k, key in zip(new, grp.keys(fb.closed_form(grp, self.g, new))):
            self.memo[k] = key
        return [self.memo[k] for k in ks]


def _expect_one(port, name):
    """the expectations for the generator of a group, shared by the tests that use it"""
    if name not in _expect:
        grp = _grp(port, name)
        _expect[name] = Expect(grp, grp.one)
    return _expect[name]


def _device(engine, grp, scalar_size, window, g, scalars, coeff=None, plain=False, out_form=OUT_LIBFF, stream=None, check=True):
    """one call on uploaded scalars: the records, with the words around them and the scalars afterwards checked"""
    n, cols = scalars.shape[0], grp.one.shape[0]
    d_sc, d_out = engine.malloc(max(16, scalars.nbytes)), engine.malloc((n * cols + 2 * PAD) * 8)
    try:
        buf = np.full(n * cols + 2 * PAD, SENTINEL, dtype=np.uint64)
        engine.h2d(d_out, buf)
        if n:
            engine.h2d(d_sc, scalars)
        cf = grp.scalars([coeff], plain)[0] if coeff is not None else None
        engine.batch_exp_device(grp.curve, grp.group, scalar_size, window, g, d_sc if n else None, n,
                                d_out.value + PAD * 8 if n else None, coeff=cf, scalars_plain=plain, out_form=out_form, stream=stream)
        engine.synchronize()
        engine.d2h(buf, d_out)
        if check:
            assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + n * cols:] == SENTINEL).all(), "sentinels around d_out"
            if n:
                back = np.zeros_like(scalars)
                engine.d2h(back, d_sc)
                assert (back == scalars).all(), "the scalars are unchanged"
        return buf[PAD:PAD + n * cols].reshape(n, cols).copy()
    finally:
        engine.free(d_sc)
        engine.free(d_out)


def _is_special(grp, rows):
    c = grp.one.shape[0] // 3
    for row in rows:
        assert (row[2 * c:] == grp.one[2 * c:]).all() or (row == grp.zero).all(), "special form: Z = one, or (0, one, 0)"


def _all_forms(engine, grp, exp, scalar_size, window, ks, coeff=None, forms=(False, True)):
    """Montgomery and plain records of the same values: OUT_LIBFF word for word what the host entry writes, OUT_AFFINE in
    special form, both the closed form as affine points"""
    want = exp.keys(ks, coeff)
    for plain in forms:
        sc = grp.scalars(ks, plain)
        cf = grp.scalars([coeff], plain)[0] if coeff is not None else None
        host = engine.batch_exp(grp.curve, grp.group, scalar_size, window, exp.g, sc, coeff=cf, scalars_plain=plain)
        got = _device(engine, grp, scalar_size, window, exp.g, sc, coeff, plain)
        assert (got == host).all(), (grp.name, scalar_size, window, plain, coeff, "OUT_LIBFF differs from amdmsm_batch_exp")
        keys = grp.keys(got)
        bad = [i for i in range(len(ks)) if keys[i] != want[i]]
        assert not bad, (grp.name, scalar_size, window, plain, coeff, len(bad), bad[:8], [hex(ks[i]) for i in bad[:4]])
        aff = _device(engine, grp, scalar_size, window, exp.g, sc, coeff, plain, out_form=OUT_AFFINE)
        _is_special(grp, aff)
        assert grp.keys(aff) == want, (grp.name, scalar_size, window, plain, coeff, "OUT_AFFINE")


SHAPES = ["b-w1", "b-w5", "65-w16", "1-w1"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_shapes_sizes_and_forms(engine, port, name, shape):
    """(bits, 1), (bits, 5) and (65, 16) at every n of WORKGROUP_NS, (1, 1) at n = 1 with both of its values: the edge
    scalars of each shape (zero digits in every position, single powers, r - 1), values below r so that both record forms
    hold them; n = 1 takes the last of the sixteen values of its shape"""
    grp, exp = _grp(port, name), _expect_one(port, name)
    if shape == "1-w1":
        for k in (0, 1):
            _all_forms(engine, grp, exp, 1, 1, [k])
        return
    scalar_size, window = {"b-w1": (grp.bits, 1), "b-w5": (grp.bits, 5), "65-w16": (65, 16)}[shape]
    for n in fb.WORKGROUP_NS:
        ks = fb.scalar_values(scalar_size, window, grp.r, seed=n, n=max(n, 16), below_r=True)[-n:]
        _all_forms(engine, grp, exp, scalar_size, window, ks)


@pytest.mark.parametrize("name", fb.ALL_GROUPS)
def test_coefficients(engine, port, name):
    """coeff 0 (every result zero), 1, r - 1 (the negatives); the plain path converts both factors before it multiplies"""
    grp, exp = _grp(port, name), _expect_one(port, name)
    ks = fb.scalar_values(grp.bits, 5, grp.r, seed=255, n=255, below_r=True)   # the values of the b-w5 case: kept
    plain_results = fb.closed_form(grp, grp.one, ks[:16])
    assert exp.keys(ks[:16], coeff=0) == grp.keys([grp.zero] * 16)
    assert exp.keys(ks[:16], coeff=grp.r - 1) == grp.keys([grp.neg(x) for x in plain_results])
    for coeff in (0, 1, grp.r - 1):
        _all_forms(engine, grp, exp, grp.bits, 5, ks, coeff=coeff)


def test_out_jacobian_and_the_other_refusals(engine, port):
    grp = _grp(port, "alt_bn128_g1")
    ks = [1, 2, 3, 4]
    sc = grp.scalars(ks, False)
    d_sc, d_out = engine.malloc(1024), engine.malloc(4096)
    try:
        buf = np.full(512, SENTINEL, dtype=np.uint64)
        engine.h2d(d_out, buf)
        engine.h2d(d_sc, sc)
        s, o = d_sc.value, d_out.value
        call = lambda ds, do, n=4, g=grp.one, size=grp.bits, w=5, **kw: engine.batch_exp_device(grp.curve, grp.group, size, w, g, ds, n, do, **kw)
        for args, kw, text in (((s, o), {"out_form": OUT_JACOBIAN}, "out_form"),
                               ((None, o), {}, "null pointer"), ((s, None), {}, "null pointer"),
                               ((s, o, 4, None), {}, "null pointer"),
                               ((s + 8, o), {}, "d_scalars: not aligned to 16 bytes"),
                               ((s, o + 8), {}, "d_out_xyz: not aligned to 16 bytes"),
                               ((s, s + 64), {}, "d_out_xyz overlaps d_scalars"), ((s, s), {}, "d_out_xyz overlaps d_scalars"),
                               ((o + 96, o), {}, "d_out_xyz overlaps d_scalars"),
                               ((s, o, 4, grp.one, grp.bits, 0), {}, "window / scalar_size"),
                               ((s, o, 4, grp.one, grp.bits, 23), {}, "window / scalar_size"),
                               ((s, o, 4, grp.one, 0), {}, "window / scalar_size"),
                               ((s, o, 4, grp.one, 64 * grp.limbs + 1), {}, "window / scalar_size")):
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                call(*args, **kw)
            assert ei.value.code == BAD_ARG and text in str(ei.value), (args, kw, str(ei.value))
        o_bad = engine._opts()
        o_bad.struct_size += 4
        rc = engine.lib.amdmsm_batch_exp_device(engine.h, grp.curve, grp.group, ctypes.c_size_t(grp.bits), ctypes.c_size_t(5),
                                                grp.one.ctypes.data_as(ctypes.c_void_p), d_sc, ctypes.c_size_t(4), None, d_out,
                                                ctypes.byref(o_bad))
        assert rc == BAD_ARG and b"struct_size" in engine.lib.amdmsm_last_error(engine.h)
        with pytest.raises(libff_amd.AmdMsmError) as ei:
            engine.batch_exp_device(5, 2, 64, 5, grp.one, s, 4, o)
        assert ei.value.code == UNSUPPORTED
        engine.synchronize()
        engine.d2h(buf, d_out)
        assert (buf == SENTINEL).all(), "a refused call writes nothing"
        back = np.zeros_like(sc)
        engine.d2h(back, d_sc)
        assert (back == sc).all()
        # the 10-word fields: 8 bytes
        mnt = _grp(port, "mnt4_g1")
        with pytest.raises(libff_amd.AmdMsmError) as ei:
            engine.batch_exp_device(mnt.curve, mnt.group, mnt.bits, 5, mnt.one, s + 4, 4, o)
        assert ei.value.code == BAD_ARG and "d_scalars: not aligned to 8 bytes" in str(ei.value)
    finally:
        engine.free(d_sc)
        engine.free(d_out)


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_377_g2", "mnt6_g1"])
def test_table_sharing_and_n_zero(port, name):
    """One context: a table built by the host entry serves the device entry (ms[1] == 0) and the other way round; another
    g rebuilds it; n = 0 builds or keeps it and writes nothing; a call on a second stream right behind a build on the
    first reads the finished table."""
    grp = _grp(port, name)
    b = grp.bits
    g2 = grp.multiple_not_normalised(4242)
    e1, e2 = _expect_one(port, name), Expect(grp, g2)
    ks = fb.scalar_values(b, 9, grp.r, seed=3, n=64, below_r=True)
    sc = grp.scalars(ks, False)
    eng = libff_amd.Engine(0)
    try:
        def device(g, exp, stream=None, n=64):
            got = _device(eng, grp, b, 9, g, sc[:n], stream=stream)
            ms = eng.batch_exp_timings()
            assert grp.keys(got) == exp.keys(ks[:n])
            assert ms["d2h_ms"] == 0, "OUT_LIBFF: no normalisation"
            return ms["table_ms"]

        def host(g, exp):
            got = eng.batch_exp(grp.curve, grp.group, b, 9, g, sc)
            assert grp.keys(got) == exp.keys(ks)
            return eng.batch_exp_timings()["table_ms"]

        assert host(grp.one, e1) > 0
        assert device(grp.one, e1) == 0, "the host entry's table serves the device entry"
        assert device(g2, e2) > 0, "another g: rebuilt"
        assert device(g2, e2) == 0
        assert host(g2, e2) == 0, "the device entry's table serves the host entry"
        assert device(grp.one, e1, n=0) > 0, "n = 0 builds"
        assert device(grp.one, e1, n=0) == 0, "n = 0 keeps"
        assert host(grp.one, e1) == 0
        aff = _device(eng, grp, b, 9, grp.one, sc, out_form=OUT_AFFINE)
        ms = eng.batch_exp_timings()
        assert ms["table_ms"] == 0 and ms["d2h_ms"] > 0 and ms["exp_ms"] > 0
        _is_special(grp, aff)
        # build on one stream, use on another, nothing waited for in between
        hip, streams = hip_runtime(), [ctypes.c_void_p(), ctypes.c_void_p()]
        for st in streams:
            assert hip.hipStreamCreate(ctypes.byref(st)) == 0
        cols = grp.one.shape[0]
        d_sc, d_a, d_b = eng.malloc(sc.nbytes), eng.malloc(64 * cols * 8), eng.malloc(64 * cols * 8)
        try:
            eng.h2d(d_sc, sc)
            eng.batch_exp_device(grp.curve, grp.group, b, 10, g2, d_sc, 64, d_a, stream=streams[0])
            eng.batch_exp_device(grp.curve, grp.group, b, 10, g2, d_sc, 64, d_b, stream=streams[1])
            assert eng.batch_exp_timings()["table_ms"] == 0
            eng.synchronize()
            for d in (d_a, d_b):
                got = np.zeros((64, cols), dtype=np.uint64)
                eng.d2h(got, d)
                assert grp.keys(got) == e2.keys(ks)
        finally:
            eng.synchronize()
            for p in (d_sc, d_a, d_b):
                eng.free(p)
            for st in streams:
                assert hip.hipStreamDestroy(st) == 0
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_377_g2", "mnt4_g1"])
def test_powers_of_tau_to_a_file(engine, port, name, tmp_path):
    """fr_powers_device(t, 193) -> batch_exp_device -> import_bases_device -> write_points_file -> multi_exp_stream_file
    with scalars s: (sum s_i t^i mod r) G.  Through OUT_LIBFF / form normal and through OUT_AFFINE / form special."""
    grp = _grp(port, name)
    n, rng = 193, random.Random(193)
    t = rng.randrange(2, grp.r)
    s_int = [rng.randrange(grp.r) for _ in range(n)]
    want = grp.keys([grp.mul(sum(s * pow(t, i, grp.r) for i, s in enumerate(s_int)) % grp.r, grp.one)])[0]
    scal = grp.scalars(s_int, True)
    sz = libff_amd.sizes(grp.curve, grp.group)
    d_pow, d_xyz, d_aff = engine.malloc(n * sz["fr_bytes"]), engine.malloc(n * sz["g_bytes"]), engine.malloc(n * sz["affine_bytes"])
    try:
        engine.fr_powers_device(grp.curve, t, n, d_pow)
        for out_form, base_form in ((OUT_LIBFF, libff_amd.multi_exp_base_form_normal), (OUT_AFFINE, libff_amd.multi_exp_base_form_special)):
            engine.batch_exp_device(grp.curve, grp.group, grp.bits, 7, grp.one, d_pow, n, d_xyz, out_form=out_form)
            engine.import_bases_device(grp.curve, grp.group, d_xyz, sz["g_bytes"], base_form, n, d_aff)
            path = str(tmp_path / f"srs_{out_form}.bin")
            engine.write_points_file(grp.curve, grp.group, d_aff, n, path, chunk_points=64)
            got = engine.multi_exp_stream_file(grp.curve, grp.group, path, scal, chunk_points=64, scalars_plain=True)
            assert grp.keys([got])[0] == want, (name, out_form)
    finally:
        engine.synchronize()
        for p in (d_pow, d_xyz, d_aff):
            engine.free(p)
