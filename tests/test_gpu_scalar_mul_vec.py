"""Element-wise scalar multiplication out[i] = k_i * P_i on the device (Engine.scalar_mul_vec / scalar_mul_vec_device), all
eleven groups.  Expected values: oracle.port.scalar_mul for the eight pairing-curve groups, tests/mnt_model.py for the
three MNT groups; everything is compared in affine form (special-form records, bit for bit).  Nothing here knows the
window width of the ladder: the edge scalars put the running sum at +-(table entry) in the last step for any width up to 5.

An MNT vector holds at most 96 different elements, because the Python model computes their multiples; the 257-element
cases repeat them."""
import ctypes
import random

import numpy as np
import pytest

import mnt_model as mm
from common import GROUPS, golden, to_int

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G1, G2, MNT4, MNT6, OUT_AFFINE, OUT_LIBFF, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special)

BAD_ARG, UNSUPPORTED = -2, -3
ALL = [pytest.param(name, id=name) for name, _, _ in GROUPS] + [pytest.param(n, id=n) for n in ("mnt4_g1", "mnt4_g2", "mnt6_g1")]
N_BIG = 257
SIZES = [0, 1, 63, 64, 65, N_BIG]
EDGE_SMALL = [0, 1, 2, 7, 8, 9, 15, 16, 17, 1 << 31, 1 << 32, (1 << 64) - 1]


def _words(v, n):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(n)], dtype=np.uint64)


class PairingGroup:
    """records and expected values through the plain-C restatement"""
    distinct = N_BIG

    def __init__(self, port, name, curve, group):
        self.port, self.name, self.curve, self.group = port, name, curve, group
        s = port.sizes(curve, group)
        self.fl, self.gl = s["fr_bytes"] // 8, s["g_bytes"] // 8
        self.cl = self.gl // 3
        self.r = to_int(golden()[f"{libff_amd.engine.CURVE_NAMES[curve]}_g1/fr_modulus"])
        self.one, self.zero = port.group_consts(curve, group)
        self.projective = curve == 2   # bw6_761 records are homogeneous projective

    def points(self, n):
        return self.port.bases_seq(self.curve, self.group, n, first=2)

    def neg(self, rec):
        return self.port.group_op(self.curve, self.group, 3, rec)

    def infinity(self):
        return self.zero.copy()

    def scale(self, recs, seed):
        """the same points with a random Z each (normal base form)"""
        rng = random.Random(seed)
        cl, out = self.cl, recs.copy()
        mul = lambda a, b: self.port.fq_op(self.curve, self.group, 0, a, b)
        for i, rec in enumerate(recs):
            if not rec[2 * cl:].any():
                continue
            z = recs[rng.randrange(len(recs))][:cl]   # a coordinate of some point: a random nonzero field element
            if not z.any():
                continue
            z2 = mul(z, z)
            if self.projective:
                out[i, :cl], out[i, cl:2 * cl] = mul(rec[:cl], z), mul(rec[cl:2 * cl], z)
            else:
                out[i, :cl], out[i, cl:2 * cl] = mul(rec[:cl], z2), mul(rec[cl:2 * cl], mul(z2, z))
            out[i, 2 * cl:] = z
        return out

    def mont(self, ks):
        return self.port.fr_from_bigint(self.curve, np.stack([_words(k % self.r, self.fl) for k in ks]))

    def plain(self, ks):
        return np.stack([_words(k, self.fl) for k in ks])

    def expected(self, recs, ks):
        """special-form records of k_i * P_i"""
        sc = self.mont(ks)
        return np.stack([self.port.group_op(self.curve, self.group, 4, self.port.scalar_mul(self.curve, self.group, recs[i], sc[i]))
                         for i in range(len(ks))])

    def special(self, got):
        return self.port.batch_to_special(self.curve, self.group, got)


class MntGroup:
    """records and expected values through the integer model"""
    distinct = 96

    def __init__(self, name, curve, group, model):
        self.name, self.curve, self.group, self.model = name, curve, group, model
        self.r, self.fl, self.gl = model.r, mm.WORDS, 3 * model.cw
        self._pts = {}

    def _remember(self, recs, pts):
        for rec, P in zip(recs, pts):
            self._pts[rec.tobytes()] = P
        return recs

    def points(self, n):
        m = self.model
        pts, P = [], m.mul(3, m.one)
        for _ in range(min(n, self.distinct)):
            pts.append(P)
            P = m.add(P, m.one)
        pts = [pts[i % self.distinct] for i in range(n)]
        return self._remember(m.records(pts), pts)

    def neg(self, rec):
        P = self.model.neg(self._pts[rec.tobytes()])
        return self._remember(self.model.records([P]), [P])[0]

    def infinity(self):
        return self._remember(self.model.records([mm.INF]), [mm.INF])[0]

    def scale(self, recs, seed):
        rng = random.Random(seed)
        pts = [self._pts[r.tobytes()] for r in recs]
        return self.model.records(pts, [rng.randrange(1, self.model.p) for _ in pts])

    def mont(self, ks):
        return self.model.scalars_mont(ks)

    def plain(self, ks):
        return np.stack([_words(k, self.fl) for k in ks])

    def expected(self, recs, ks):
        m, memo, out = self.model, {}, []
        for rec, k in zip(recs, ks):
            key = (rec.tobytes(), k % m.r)
            if key not in memo:
                P, kk = self._pts[rec.tobytes()], k % m.r
                memo[key] = m.neg(m.mul(m.r - kk, P)) if kk > m.r // 2 else m.mul(kk, P)   # near r: a short multiple
            out.append(memo[key])
        return m.records(out)

    def special(self, got):
        return self.model.records([self.model.point(r) for r in got])


_groups = {}


def group_of(port, name):
    if name not in _groups:
        pairing = {g[0]: g for g in GROUPS}
        if name in pairing:
            _groups[name] = PairingGroup(port, *pairing[name])
        else:
            curve, group, model = {"mnt4_g1": (MNT4, G1, mm.MNT4), "mnt4_g2": (MNT4, G2, mm.MNT4_G2),
                                   "mnt6_g1": (MNT6, G1, mm.MNT6)}[name]
            _groups[name] = MntGroup(name, curve, group, model)
    return _groups[name]


_vectors = {}


def vector(port, name):
    """(group, special-form points, scalars as integers, expected special-form records) of the 257-element case: computed
    once per group, shared by the tests below and never changed"""
    if name not in _vectors:
        g = group_of(port, name)
        recs = g.points(N_BIG)
        rng = random.Random(sum(name.encode()))
        ks = [rng.randrange(g.r) for _ in range(g.distinct)]
        ks = [ks[i % g.distinct] for i in range(N_BIG)]
        want = g.expected(recs[:g.distinct], ks[:g.distinct])
        want = np.stack([want[i % g.distinct] for i in range(N_BIG)])
        for a in (recs, want):
            a.setflags(write=False)
        _vectors[name] = (g, recs, ks, want)
    return _vectors[name]


def run(engine, g, recs, sc, **kw):
    """the host entry, result in special form whatever the output form"""
    out_form = kw.get("out_form", OUT_LIBFF)
    got = engine.scalar_mul_vec(g.curve, g.group, recs, sc, **kw)
    return got if out_form == OUT_AFFINE or len(got) == 0 else g.special(got)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine, port, name, n):
    g, recs, ks, want = vector(port, name)
    got = run(engine, g, recs[:n], g.mont(ks[:n]) if n else np.zeros((0, g.fl), dtype=np.uint64),
              base_form=multi_exp_base_form_special, out_form=OUT_AFFINE)
    assert got.shape == (n, g.gl)
    assert (got == want[:n]).all()


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("chunk", [1, 64, 100])
def test_chunks_equal_the_automatic_split(engine, port, name, chunk):
    """the last chunk partial (64, 100), a chunk of one element"""
    g, recs, ks, want = vector(port, name)
    sc = g.mont(ks)
    auto = engine.scalar_mul_vec(g.curve, g.group, recs, sc, base_form=multi_exp_base_form_special, out_form=OUT_AFFINE)
    got = engine.scalar_mul_vec(g.curve, g.group, recs, sc, base_form=multi_exp_base_form_special, out_form=OUT_AFFINE,
                                chunk_points=chunk)
    assert (got == auto).all() and (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_base_forms_output_forms_and_scalar_forms(engine, port, name):
    g, recs, ks, want = vector(port, name)
    n = 65
    normal = g.scale(recs[:n], seed=11)
    assert (normal != recs[:n]).any()
    for base_form, pts in ((multi_exp_base_form_special, recs[:n]), (multi_exp_base_form_normal, normal)):
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            for plain in (False, True):
                sc = g.plain(ks[:n]) if plain else g.mont(ks[:n])
                got = run(engine, g, pts, sc, base_form=base_form, out_form=out_form, scalars_plain=plain)
                assert (got == want[:n]).all(), (base_form, out_form, plain)


@pytest.mark.parametrize("name", ALL)
def test_edge_scalars(engine, port, name):
    """Small scalars, powers of two, r - 2, r - 1 in both scalar forms; as plain integers also the whole sweep r - 40 .. r + 40
    -- the running sum meets +-(table entry) in the last step: the equal-point and the opposite-point branch of the adder --
    and the all-ones scalar, whose top window carries out.  A plain scalar >= r gives (k mod r) P."""
    g, recs, _, _ = vector(port, name)
    P = recs[5]
    ks = EDGE_SMALL + [g.r - 2, g.r - 1]
    pts = np.stack([P] * len(ks))
    want = g.expected(pts, ks)
    for plain in (False, True):
        got = run(engine, g, pts, g.plain(ks) if plain else g.mont(ks), base_form=multi_exp_base_form_special,
                  out_form=OUT_AFFINE, scalars_plain=plain)
        assert (got == want).all(), plain
    ks = list(range(g.r - 40, g.r + 41)) + [(1 << (64 * g.fl)) - 1]
    pts = np.stack([P] * len(ks))
    want = g.expected(pts, ks)
    for out_form in (OUT_AFFINE, OUT_LIBFF):
        got = run(engine, g, pts, g.plain(ks), base_form=multi_exp_base_form_special, out_form=out_form, scalars_plain=True)
        bad = [k - g.r for k, a, b in zip(ks, got, want) if (a != b).any()]
        assert not bad, f"wrong at r + {bad}"


@pytest.mark.parametrize("name", ALL)
def test_edge_points(engine, port, name):
    """Infinity with zero and nonzero scalars in both base forms; P and -P with equal scalars; one point in every lane of a
    wave with different scalars."""
    g, recs, ks, _ = vector(port, name)
    inf, P = g.infinity(), recs[0]
    pts = np.stack([inf, inf, inf, P, g.neg(P), P, g.neg(P)] + [recs[7]] * 64)
    k = ks[3]
    sc = [0, 5, g.r - 1, k, k, 1, 1] + [ks[i % g.distinct] if i % 2 else i + 1 for i in range(64)]
    want = g.expected(pts, sc)
    assert (want[3, :g.gl // 3] == want[4, :g.gl // 3]).all() and (want[3] != want[4]).any()   # k P and k (-P): same x
    for base_form in (multi_exp_base_form_special, multi_exp_base_form_normal):
        src = pts if base_form == multi_exp_base_form_special else g.scale(pts, seed=12)
        got = run(engine, g, src, g.mont(sc), base_form=base_form, out_form=OUT_AFFINE)
        assert (got == want).all(), base_form
        got = run(engine, g, src, g.mont(sc), base_form=base_form, out_form=OUT_LIBFF)
        assert (got == want).all(), base_form


@pytest.mark.parametrize("name", ALL)
def test_cross_check_against_multi_exp(engine, port, name):
    """sum of the outputs = multi_exp(points, scalars) of the inputs, 64 random elements"""
    g, recs, ks, _ = vector(port, name)
    n = 64
    sc = g.mont(ks[:n])
    outs = engine.scalar_mul_vec(g.curve, g.group, recs[:n], sc, base_form=multi_exp_base_form_special, out_form=OUT_LIBFF)
    lhs = engine.multi_exp(g.curve, g.group, outs, g.mont([1] * n), base_form=multi_exp_base_form_normal, out_form=OUT_AFFINE)
    rhs = engine.multi_exp(g.curve, g.group, recs[:n], sc, base_form=multi_exp_base_form_special, out_form=OUT_AFFINE)
    assert (lhs == rhs).all()
    assert lhs[2 * (g.gl // 3):].any(), "the sum is not expected to be zero"


def _hip_runtime():
    """the HIP runtime the engine library has loaded, for a stream of the caller's own"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "the engine library is loaded with its HIP runtime"
    lib = ctypes.CDLL(sorted(paths)[0])
    lib.hipStreamSynchronize.argtypes = lib.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("name", ALL)
def test_device_entry(engine, port, name):
    """the host case on resident inputs: malloc / h2d, points made on the device by gen_bases_seq_device ((first + i + 1) G),
    chunked and on a stream of the caller's"""
    g, recs, ks, _ = vector(port, name)
    n = g.distinct
    s = libff_amd.sizes(g.curve, g.group)
    sc = g.mont(ks[:n])
    # the same points as special-form records, for the expected values: export_affine of the resident points
    d_aff, d_sc, d_out = engine.malloc(n * s["affine_bytes"]), engine.malloc(sc.nbytes), engine.malloc(n * s["g_bytes"])
    try:
        engine.gen_bases_seq_device(g.curve, g.group, 2, n, d_aff)
        engine.h2d(d_sc, sc)
        engine.export_affine_device(g.curve, g.group, d_aff, n, d_out)
        engine.synchronize()
        pts = np.zeros((n, g.gl), dtype=np.uint64)
        engine.d2h(pts, d_out)
        assert (pts == recs[:n]).all()   # vector() starts at 3 G as well
        want = vector(port, name)[3][:n]
        hip, stream = _hip_runtime(), ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        for out_form, chunk, st in ((OUT_AFFINE, 0, None), (OUT_LIBFF, 40, None), (OUT_AFFINE, 64, stream)):
            engine.scalar_mul_vec_device(g.curve, g.group, d_aff, d_sc, n, d_out, out_form=out_form, chunk_points=chunk, stream=st)
            if st is not None:
                assert hip.hipStreamSynchronize(st) == 0   # the call ran on the caller's stream: nothing else is waited for
            else:
                engine.synchronize()
            got = np.zeros((n, g.gl), dtype=np.uint64)
            engine.d2h(got, d_out)
            assert ((got if out_form == OUT_AFFINE else g.special(got)) == want).all(), (out_form, chunk)
        assert hip.hipStreamDestroy(stream) == 0
    finally:
        for p in (d_aff, d_sc, d_out):
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_refused_calls_leave_the_output_alone(engine, port, name):
    g, recs, ks, _ = vector(port, name)
    n = 4
    sc = g.mont(ks[:n])
    s = libff_amd.sizes(g.curve, g.group)
    out = np.full((n, g.gl), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    wide = np.zeros((n, g.gl + 1), dtype=np.uint64)
    wide[:, :g.gl] = recs[:n]
    o = engine._opts(out_form=OUT_AFFINE)
    call = lambda curve, group, pts, stride, scal, dst: engine.lib.amdmsm_scalar_mul_vec(
        engine.h, curve, group, pts, ctypes.c_size_t(stride), multi_exp_base_form_special, scal, ctypes.c_size_t(n), dst,
        ctypes.c_size_t(0), ctypes.byref(o))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # a stride that is no multiple of the record alignment (4 bytes more than a record), one shorter than a record
    assert call(g.curve, g.group, ptr(wide), s["g_bytes"] + 4, ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, ptr(wide), s["g_bytes"] - 16, ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, None, s["g_bytes"], ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, ptr(wide), s["g_bytes"], None, ptr(out)) == BAD_ARG
    assert call(MNT6, G2, ptr(wide), s["g_bytes"], ptr(sc), ptr(out)) == UNSUPPORTED
    assert engine.lib.amdmsm_scalar_mul_vec_device(engine.h, MNT6, G2, None, None, ctypes.c_size_t(n), None, ctypes.c_size_t(0),
                                                   ctypes.byref(o)) == UNSUPPORTED
    assert (out == 0x5a5a5a5a5a5a5a5a).all()
    # a padded stride that keeps the alignment is accepted
    got = engine.scalar_mul_vec(g.curve, g.group, np.concatenate([wide, wide], axis=1)[:, :2 * g.gl], sc,
                                base_form=multi_exp_base_form_special, out_form=OUT_AFFINE, stride_bytes=2 * s["g_bytes"])
    assert (got == vector(port, name)[3][:n]).all()
