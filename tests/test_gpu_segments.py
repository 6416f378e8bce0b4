"""Segmented MSM out[j] = sum of k_i * P_i over segment j on the device (Engine.multi_exp_segments / msm_device_segments),
all eleven groups.  Expected values: the products k_i * P_i of tests/test_gpu_scalar_mul_vec.py's vector (oracle.port for
the eight pairing-curve groups, tests/mnt_model.py for the three MNT groups) added up per segment by the same oracles
(tests/segments_model.py); everything is compared as special-form records, bit for bit.  Nothing here knows the window
width or the lane mapping of the kernels: the segment counts are odd, so the lane count is no multiple of 64 for any
number of windows per scalar that is odd (65, 81, 97)."""
import ctypes

import numpy as np
import pytest

import segments_model as sm
from segments_model import ALL, LENS_65, LENS_SMALL, SIZE_MAX

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G2, MNT6, OUT_AFFINE, OUT_LIBFF, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special)

BAD_ARG, UNSUPPORTED = -2, -3
SPECIAL = multi_exp_base_form_special


def run(engine, g, recs, sc, offs, **kw):
    """the host entry, result in special form whatever the output form"""
    kw.setdefault("base_form", SPECIAL)
    kw.setdefault("out_form", OUT_AFFINE)
    got = engine.multi_exp_segments(g.curve, g.group, recs, sc, offs, **kw)
    return got if kw["out_form"] == OUT_AFFINE or len(got) == 0 else g.special(got)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("m", [0, 1, 2, 65])
def test_shapes(engine, port, name, m):
    """m segments of mixed lengths (empty ones first, last and adjacent at m = 65), terms in front of the first segment and
    behind the last one"""
    lens = {0: [], 1: [65], 2: [63, 257], 65: LENS_65}[m]
    g, recs, ks, offs, want = sm.case(port, name, lens, first=3, slack=5)
    assert offs[0] > 0 and offs[-1] < len(recs) and len(offs) == m + 1
    got = run(engine, g, recs, g.mont(ks), offs)
    assert got.shape == (m, g.gl)
    bad = [j for j in range(m) if (got[j] != want[j]).any()]
    assert not bad, f"wrong segments {bad} (lengths {[lens[j] for j in bad]})"


@pytest.mark.parametrize("name", ALL)
def test_adder_edges_inside_a_window_sum(engine, port, name):
    """Every special case of the mixed addition met inside one lane's chain, alone and beside ordinary terms: the equal
    point, the opposite point, an infinite base with zero and nonzero scalars, a zero scalar, a total of infinity."""
    g, recs, ks, _ = sm.vector(port, name)
    P, Q1, Q2, inf = recs[0], recs[1], recs[2], g.infinity()
    nP, nQ1 = g.neg(P), g.neg(Q1)
    k, k1, k2 = ks[0], ks[1], ks[2]
    segs = [
        [(P, k), (P, k)], [(Q1, k1), (P, k), (P, k), (Q2, k2)],                    # equal point
        [(P, k), (nP, k)], [(Q1, k1), (P, k), (nP, k), (Q2, k2)],                  # opposite point
        [(inf, 5)], [(inf, 0), (inf, 5), (Q1, k1)], [(Q1, k1), (inf, g.r - 1), (Q2, k2)],
        [(Q1, 0)], [(Q1, 0), (Q2, k2)], [(Q1, k1), (Q2, 0), (P, k)],                 # zero scalar
        [(P, k), (Q1, k1), (nP, k), (nQ1, k1)],                                    # total of infinity
    ]
    pts = np.stack([p for s in segs for p, _ in s])
    sc = [c for s in segs for _, c in s]
    offs = sm.offsets_of([len(s) for s in segs])
    want = sm.Sums(g, port).segments(g.expected(pts, sc), offs)
    zero = sm.Sums(g, port).segments(pts[:0], sm.offsets_of([0]))[0]
    for j in (2, 4, 7, 10):
        assert (want[j] == zero).all()
    assert (want[1] != zero).any() and (want[3] != zero).any()
    for plain in (False, True):
        got = run(engine, g, pts, g.plain(sc) if plain else g.mont(sc), offs, scalars_plain=plain, long_from=SIZE_MAX)
        bad = [j for j in range(len(segs)) if (got[j] != want[j]).any()]
        assert not bad, (plain, bad)


@pytest.mark.parametrize("name", ALL)
def test_edge_scalars(engine, port, name):
    """The edge scalars of the element-wise tests as single-term segments and as two-term segments beside an ordinary term:
    small values, powers of two, r - 2, r - 1 in both scalar forms; as plain integers also r - 40 .. r + 40 and the
    all-ones word pattern, whose top window carries out.  A plain scalar >= r means k mod r."""
    g, recs, ks, vec_want = sm.vector(port, name)
    P, Q, kq = recs[5], recs[6], ks[6]
    sums = sm.Sums(g, port)

    def check(edge, plain):
        n = len(edge)
        pts = np.stack([P] * n + [P, Q] * n)
        sc = list(edge) + [c for k in edge for c in (k, kq)]
        offs = np.concatenate([np.arange(n), n + 2 * np.arange(n + 1)]).astype(np.uint64)
        prods = np.concatenate([g.expected(pts[:n], edge), vec_want[6:7]])
        want = sums.segments(prods, offs, column=lambda j, i: i if i < n else ((i - n) // 2 if (i - n) % 2 == 0 else n))
        got = run(engine, g, pts, g.plain(sc) if plain else g.mont(sc), offs, scalars_plain=plain)
        bad = [(j % n, edge[j % n] - g.r) for j in range(2 * n) if (got[j] != want[j]).any()]
        assert not bad, f"plain={plain}: wrong at (index, k - r) {bad}"

    for plain in (False, True):
        check(sm.EDGE_SMALL + [g.r - 2, g.r - 1], plain)
    check(list(range(g.r - 40, g.r + 41)) + [(1 << (64 * g.fl)) - 1], True)


@pytest.mark.parametrize("name", ALL)
def test_base_forms_output_forms_and_stride(engine, port, name):
    g, recs, ks, offs, want = sm.case(port, name, LENS_SMALL[:8], first=1, slack=2)
    sc = g.mont(ks)
    normal = g.scale(recs, seed=21)
    assert (normal != recs).any()
    for base_form, pts in ((SPECIAL, recs), (multi_exp_base_form_normal, normal)):
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            got = run(engine, g, pts, sc, offs, base_form=base_form, out_form=out_form)
            assert (got == want).all(), (base_form, out_form)
    # a padded stride that keeps the alignment
    s = libff_amd.sizes(g.curve, g.group)
    wide = np.zeros((len(recs), 2 * g.gl), dtype=np.uint64)
    wide[:, :g.gl] = recs
    got = run(engine, g, wide, sc, offs, stride_bytes=2 * s["g_bytes"])
    assert (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_shared_bases(engine, port, name):
    """65 scalar vectors of lengths 1 .. 65 over one vector of 65 points: equal to the unshared call on the repeated
    bases, and to the oracle.  The scalar of a term depends on its segment, so a term read from another segment shows."""
    g, recs, ks, vec_want = sm.vector(port, name)
    nb = 65
    lens = list(range(1, nb + 1))
    offs = sm.offsets_of(lens)
    own = lambda j, i: (i + j) % 3 != 0    # the vector's own scalar (product known), else a small one
    sc, cols = [], []
    for j, ln in enumerate(lens):
        sc += [ks[i] if own(j, i) else 1 + (i + 2 * j) % 8 for i in range(ln)]
        cols += list(range(ln))
    small = g.expected(np.repeat(recs[:nb], 8, axis=0), [1 + v for _ in range(nb) for v in range(8)])
    prods = np.concatenate([vec_want[:nb], small])

    def column(j, t):
        i = t - int(offs[j])
        return i if own(j, i) else nb + 8 * i + (i + 2 * j) % 8

    want = sm.Sums(g, port).segments(prods, offs, column=column)
    scm = g.mont(sc)
    shared = run(engine, g, recs[:nb], scm, offs, shared_bases=True)
    repeated = run(engine, g, recs[cols], scm, offs)
    assert (shared == repeated).all()
    bad = [j for j in range(nb) if (shared[j] != want[j]).any()]
    assert not bad, bad
    # a shared vector longer than every segment, chunked, in the library's own record form
    got = run(engine, g, recs[:nb + 7], scm, offs, shared_bases=True, chunk_terms=100, out_form=OUT_LIBFF)
    assert (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_routing_gives_identical_records(engine, port, name):
    """long_from 1 (every segment through the single-MSM route), 64 (a mixture) and SIZE_MAX (none) on one input"""
    g, recs, ks, offs, want = sm.case(port, name, LENS_SMALL, first=0, slack=0)
    sc = g.mont(ks)
    for out_form in (OUT_AFFINE, OUT_LIBFF):
        for long_from in (1, 64, SIZE_MAX):
            got = run(engine, g, recs, sc, offs, long_from=long_from, out_form=out_form)
            assert (got == want).all(), (out_form, long_from)
    shared_offs = sm.offsets_of([3, 65, 64, 0, 63])
    n = int(shared_offs[-1])
    outs = [run(engine, g, recs[:65], sc[:n], shared_offs, shared_bases=True, long_from=lf) for lf in (1, 64, SIZE_MAX)]
    assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all()


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("chunk", [1, 100, 300])
def test_chunks_equal_the_automatic_split(engine, port, name, chunk):
    """a chunk per segment (1: every segment is longer, or empty), chunks that end inside the run of segments, and a
    segment that is longer than the chunk"""
    g, recs, ks, offs, want = sm.case(port, name, LENS_SMALL, first=0, slack=0)
    sc = g.mont(ks)
    auto = run(engine, g, recs, sc, offs, long_from=SIZE_MAX)
    got = run(engine, g, recs, sc, offs, long_from=SIZE_MAX, chunk_terms=chunk)
    assert (got == auto).all() and (got == want).all()
    got = run(engine, g, recs, sc, offs, long_from=64, chunk_terms=chunk, out_form=OUT_LIBFF)
    assert (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_cross_check_against_multi_exp_and_scalar_mul_vec(engine, port, name):
    g, recs, ks, _ = sm.vector(port, name)
    n = 65
    sc = g.mont(ks[:n])
    one = run(engine, g, recs[:n], sc, np.array([0, n], dtype=np.uint64), long_from=SIZE_MAX)
    msm = engine.multi_exp(g.curve, g.group, recs[:n], sc, base_form=SPECIAL, out_form=OUT_AFFINE)
    assert (one[0] == msm).all() and one[0, 2 * (g.gl // 3):].any()
    units = run(engine, g, recs[:n], sc, np.arange(n + 1, dtype=np.uint64))
    smv = engine.scalar_mul_vec(g.curve, g.group, recs[:n], sc, base_form=SPECIAL, out_form=OUT_AFFINE)
    assert (units == smv).all()


@pytest.mark.parametrize("name", ALL)
def test_device_entry(engine, port, name):
    """resident inputs (points made on the device by gen_bases_seq_device), both routes, chunked, shared bases, and on a
    stream of the caller's"""
    g, recs, ks, vec_want = sm.vector(port, name)
    n = g.distinct
    s = libff_amd.sizes(g.curve, g.group)
    sc = g.mont(ks[:n])
    lens = [0, 3, 64, 1, 0, 2, n - 70 - 1, 0]
    offs = sm.offsets_of(lens, first=1)
    m = len(lens)
    assert offs[-1] == n
    sums = sm.Sums(g, port)
    want = sums.segments(vec_want[:n], offs)
    shared_offs = sm.offsets_of([5, 0, 64, 20])
    d_aff, d_sc, d_out = engine.malloc(n * s["affine_bytes"]), engine.malloc(sc.nbytes), engine.malloc(m * s["g_bytes"])
    try:
        engine.gen_bases_seq_device(g.curve, g.group, 2, n, d_aff)   # vector() starts at 3 G as well
        engine.h2d(d_sc, sc)
        hip, stream = sm._hip_runtime(), ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        for out_form, long_from, chunk, st in ((OUT_AFFINE, 0, 0, None), (OUT_LIBFF, 64, 40, None), (OUT_AFFINE, SIZE_MAX, 64, stream)):
            engine.msm_device_segments(g.curve, g.group, d_aff, n, d_sc, n, offs, d_out, out_form=out_form, long_from=long_from,
                                       chunk_terms=chunk, stream=st)
            if st is not None:
                assert hip.hipStreamSynchronize(st) == 0   # the call ran on the caller's stream: nothing else is waited for
            else:
                engine.synchronize()
            got = np.zeros((m, g.gl), dtype=np.uint64)
            engine.d2h(got, d_out)
            assert ((got if out_form == OUT_AFFINE else g.special(got)) == want).all(), (out_form, long_from, chunk)
        engine.msm_device_segments(g.curve, g.group, d_aff, n, d_sc, n, shared_offs, d_out, shared_bases=True,
                                   out_form=OUT_AFFINE, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        got = np.zeros((4, g.gl), dtype=np.uint64)
        engine.d2h(got, d_out)
        host = run(engine, g, recs[:n], sc, shared_offs, shared_bases=True)
        assert (got == host).all()
        assert hip.hipStreamDestroy(stream) == 0
    finally:
        for p in (d_aff, d_sc, d_out):
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_refused_calls_leave_the_output_alone(engine, port, name):
    g, recs, ks, _ = sm.vector(port, name)
    n, m = 6, 3
    sc = g.mont(ks[:n])
    s = libff_amd.sizes(g.curve, g.group)
    fill = 0x5a5a5a5a5a5a5a5a
    out = np.full((m, g.gl), fill, dtype=np.uint64)
    pts = np.ascontiguousarray(recs[:n])
    o = engine._opts(out_form=OUT_AFFINE)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = np.array([0, 2, 2, 6], dtype=np.uint64)

    def call(curve=g.curve, group=g.group, bases=pts, stride=s["g_bytes"], n_bases=n, scal=sc, n_terms=n, offs=good, flags=0,
             dst=out):
        return engine.lib.amdmsm_multi_exp_segments(
            engine.h, curve, group, None if bases is None else ptr(bases), ctypes.c_size_t(stride), SPECIAL,
            ctypes.c_size_t(n_bases), None if scal is None else ptr(scal), ctypes.c_size_t(n_terms),
            None if offs is None else ptr(offs), ctypes.c_size_t(m), ctypes.c_uint(flags), ctypes.c_size_t(0),
            None if dst is None else ptr(dst), ctypes.byref(o))

    def refused(code, word=None, **kw):
        assert call(**kw) == code, kw
        if word:
            assert word in engine.lib.amdmsm_last_error(engine.h).decode(), (kw, engine.lib.amdmsm_last_error(engine.h))
        assert (out == fill).all(), kw

    refused(BAD_ARG, bases=None)
    refused(BAD_ARG, scal=None)
    refused(BAD_ARG, offs=None)
    refused(BAD_ARG, dst=None)
    refused(BAD_ARG, stride=s["g_bytes"] + 4)
    refused(BAD_ARG, stride=s["g_bytes"] - 16)
    refused(BAD_ARG, "segment 1", offs=np.array([0, 3, 2, 6], dtype=np.uint64))
    refused(BAD_ARG, "segment 2", offs=np.array([0, 2, 2, 7], dtype=np.uint64))
    refused(BAD_ARG, flags=2)
    refused(BAD_ARG, flags=1 | 4)
    refused(BAD_ARG, n_bases=n - 1)                                 # without the flag n_bases is n_terms
    refused(BAD_ARG, "segment 2", flags=1, n_bases=3)               # with it, segment 2 has 4 terms
    refused(UNSUPPORTED, curve=MNT6, group=G2)
    d = ctypes.c_void_p(0)
    z = ctypes.c_size_t
    dev = lambda curve, group, offs, flags: engine.lib.amdmsm_msm_device_segments(
        engine.h, curve, group, d, z(n), d, z(n), ptr(offs), z(m), ctypes.c_uint(flags), z(0), d, ctypes.byref(o))
    assert dev(MNT6, G2, good, 0) == UNSUPPORTED
    assert dev(g.curve, g.group, good, 0) == BAD_ARG                    # null device pointers with work to do
    assert dev(g.curve, g.group, np.array([0, 3, 2, 6], dtype=np.uint64), 0) == BAD_ARG
    assert dev(g.curve, g.group, good, 8) == BAD_ARG
    assert (out == fill).all()
    # the same arguments, accepted
    assert call() == 0 and (out != fill).any()
