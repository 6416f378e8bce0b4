"""Fold of k point vectors by k shared scalars, out[i] = sum_j s_j * P_j[i] (Engine.fold_vec / fold_vec_device), all eleven
groups.  Expected values: oracle.port (scalar_mul, group addition, special form) for the eight pairing-curve groups,
tests/mnt_model.py for the three MNT groups; everything is compared as special-form records, bit for bit.  Nothing here
knows the window width of the ladder.

Every input point is a known multiple of the generator, taken from one pool per group: 32 points for an MNT group, whose
expected values the Python model computes from the multipliers (sum_j s_j a_j[i] times the generator, memoised), 64 for a
pairing-curve group, whose expected values are scalar_mul and additions of the records themselves.  Longer vectors repeat
the pool."""
import contextlib
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
KS = [1, 2, 3, 8]
EDGE_SMALL = [0, 1, 2, 7, 8, 9, 15, 16, 17, 1 << 31, 1 << 32, (1 << 64) - 1, 1 << 127]
FIRST = 2   # the pool starts at (FIRST + 1) G, as gen_bases_seq_device(first=FIRST) does
SPECIAL, NORMAL = multi_exp_base_form_special, multi_exp_base_form_normal


def _words(v, n):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(n)], dtype=np.uint64)


class PairingGroup:
    """records and expected values through the plain-C restatement"""
    distinct = 64

    def __init__(self, port, name, curve, group):
        self.port, self.name, self.curve, self.group = port, name, curve, group
        s = port.sizes(curve, group)
        self.fl, self.gl = s["fr_bytes"] // 8, s["g_bytes"] // 8
        self.cl = self.gl // 3
        self.r = to_int(golden()[f"{libff_amd.engine.CURVE_NAMES[curve]}_g1/fr_modulus"])
        self.one, self.zero = port.group_consts(curve, group)
        self.projective = curve == 2   # bw6_761 records are homogeneous projective
        self.pool = port.bases_seq(curve, group, self.distinct, first=FIRST)
        self.pool.setflags(write=False)
        self._terms = {}

    def neg(self, rec):
        return self.port.group_op(self.curve, self.group, 3, rec)

    def dbl(self, rec):
        return self.port.group_op(self.curve, self.group, 4, self.port.group_op(self.curve, self.group, 2, rec))

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
            z = self.pool[rng.randrange(self.distinct)][:cl]   # a coordinate of some point: a random nonzero field element
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

    def _term(self, rec, k):
        key = (rec.tobytes(), k % self.r)
        if key not in self._terms:
            self._terms[key] = self.port.scalar_mul(self.curve, self.group, rec, self.mont([k])[0])
        return self._terms[key]

    def expected(self, vecs, ks):
        """special-form records of sum_j ks[j] * vecs[j][i] (vecs: special-form records)"""
        out = np.zeros((len(vecs[0]), self.gl), dtype=np.uint64)
        for i in range(len(out)):
            acc = self.zero
            for v, k in zip(vecs, ks):
                acc = self.port.group_op(self.curve, self.group, 0, acc, self._term(v[i], k))
            out[i] = self.port.group_op(self.curve, self.group, 4, acc)
        return out

    def special(self, got):
        return self.port.batch_to_special(self.curve, self.group, got)


class MntGroup:
    """records and expected values through the integer model: every record is a known multiple a of the generator, and
    an expected value is (sum_j k_j a_j mod r) G, built from a table of d 16^w G by additions alone"""
    distinct = 32

    def __init__(self, name, curve, group, model):
        self.name, self.curve, self.group, self.model = name, curve, group, model
        self.r, self.fl, self.gl = model.r, mm.WORDS, 3 * model.cw
        self._log, self._mul, self._table = {}, {0: mm.INF}, None
        self.pool = self._records([FIRST + 1 + i for i in range(self.distinct)])
        self.pool.setflags(write=False)

    def _mul_g(self, e):
        m = self.model
        e %= m.r
        if e not in self._mul:
            if e > m.r // 2:
                self._mul[e] = m.neg(self._mul_g(m.r - e))
            else:
                if self._table is None:
                    self._table, base = [], m.one
                    for _ in range((m.r.bit_length() + 3) // 4):
                        row, P = [mm.INF], mm.INF
                        for _ in range(15):
                            P = m.add(P, base)
                            row.append(P)
                        self._table.append(row)
                        base = m.add(P, base)
                acc, w, v = mm.INF, 0, e
                while v:
                    acc = m.add(acc, self._table[w][v & 15])
                    v >>= 4
                    w += 1
                self._mul[e] = acc
        return self._mul[e]

    def _records(self, logs, zs=None):
        recs = self.model.records([self._mul_g(a) for a in logs], zs)
        for rec, a in zip(recs, logs):
            self._log[rec.tobytes()] = a % self.r
        return recs

    def neg(self, rec):
        return self._records([self.r - self._log[rec.tobytes()]])[0]

    def dbl(self, rec):
        return self._records([2 * self._log[rec.tobytes()]])[0]

    def infinity(self):
        return self._records([0])[0]

    def scale(self, recs, seed):
        rng = random.Random(seed)
        return self._records([self._log[r.tobytes()] for r in recs], [rng.randrange(1, self.model.p) for _ in recs])

    def mont(self, ks):
        return self.model.scalars_mont(ks)

    def plain(self, ks):
        return np.stack([_words(k, self.fl) for k in ks])

    def expected(self, vecs, ks):
        logs = [sum(k * self._log[v[i].tobytes()] for v, k in zip(vecs, ks)) for i in range(len(vecs[0]))]
        return self.model.records([self._mul_g(e) for e in logs]) if logs else np.zeros((0, self.gl), dtype=np.uint64)

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


def pool_vector(g, j, n):
    """vector j of n special-form points: the pool from 7 j on, repeated"""
    return g.pool[[(7 * j + i) % g.distinct for i in range(n)]]


_vectors = {}


def vector(port, name, k):
    """(group, k special-form vectors, the k scalars as integers, expected special-form records) of the 257-element case
    with k vectors: computed once per group and k, shared by the tests below and never changed"""
    if (name, k) not in _vectors:
        g = group_of(port, name)
        vecs = [pool_vector(g, j, N_BIG) for j in range(k)]
        rng = random.Random(sum(name.encode()) + k)
        ks = [rng.randrange(g.r) for _ in range(k)]
        m = min(N_BIG, g.distinct)   # the vectors repeat after g.distinct elements, all with the same period
        want = g.expected([v[:m] for v in vecs], ks)
        want = want[[i % m for i in range(N_BIG)]]
        for a in vecs + [want]:
            a.setflags(write=False)
        _vectors[(name, k)] = (g, vecs, ks, want)
    return _vectors[(name, k)]


@contextlib.contextmanager
def endomorphism(engine, value):
    """amdmsm_opts.endomorphism of the calls inside; the session's engine gets its own value back"""
    saved = engine.endomorphism
    engine.endomorphism = value
    try:
        yield
    finally:
        engine.endomorphism = saved


def run(engine, g, vecs, sc, **kw):
    """the host entry, result in special form whatever the output form"""
    out_form = kw.get("out_form", OUT_LIBFF)
    got = engine.fold_vec(g.curve, g.group, vecs, sc, **kw)
    return got if out_form == OUT_AFFINE or len(got) == 0 else g.special(got)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine, port, name, k, n):
    g, vecs, ks, want = vector(port, name, k)
    got = run(engine, g, [v[:n] for v in vecs], g.mont(ks), base_form=SPECIAL, out_form=OUT_AFFINE)
    assert got.shape == (n, g.gl)
    assert (got == want[:n]).all()


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("chunk", [1, 64, 100])
def test_chunks_equal_the_automatic_split(engine, port, name, chunk):
    """the last chunk partial (64, 100), a chunk of one element (257 chunks of one latency-bound lane each: about 55 ms a
    chunk for the 24-word field, the slowest case of this file)"""
    g, vecs, ks, want = vector(port, name, 2)
    auto = engine.fold_vec(g.curve, g.group, vecs, g.mont(ks), base_form=SPECIAL, out_form=OUT_AFFINE)
    got = engine.fold_vec(g.curve, g.group, vecs, g.mont(ks), base_form=SPECIAL, out_form=OUT_AFFINE, chunk_points=chunk)
    assert (got == auto).all() and (got == want).all()


@pytest.mark.parametrize("name", ALL)
def test_base_forms_output_forms_and_scalar_forms(engine, port, name):
    g, vecs, ks, want = vector(port, name, 2)
    n = 65
    special = [v[:n] for v in vecs]
    normal = [g.scale(v, seed=11 + j) for j, v in enumerate(special)]
    assert all((a != b).any() for a, b in zip(normal, special))
    for base_form, pts in ((SPECIAL, special), (NORMAL, normal)):
        for out_form in (OUT_LIBFF, OUT_AFFINE):
            for plain in (False, True):
                sc = g.plain(ks) if plain else g.mont(ks)
                got = run(engine, g, pts, sc, base_form=base_form, out_form=out_form, scalars_plain=plain)
                assert (got == want[:n]).all(), (base_form, out_form, plain)


@pytest.mark.parametrize("name", ALL)
def test_endomorphism_values_agree(engine, port, name):
    """the pool is multiples of the generator, hence in the order-r subgroup: every amdmsm_opts.endomorphism value gives
    the same records, and plan_fold tells which of them split the scalars"""
    g, vecs, ks, want = vector(port, name, 3)
    n = 65
    pairing = g.curve not in (MNT4, MNT6)
    whole_curve = name == "alt_bn128_g1"
    for value, split in ((-1, False), (0, whole_curve), (1, pairing), (2, pairing)):
        p = libff_amd.plan_fold(g.curve, g.group, 3, n, endomorphism=value)
        assert p["endomorphism"] == split and p["rows"] == (6 if split else 3), value
        with endomorphism(engine, value):
            for plain in (False, True):
                got = run(engine, g, [v[:n] for v in vecs], g.plain(ks) if plain else g.mont(ks), base_form=SPECIAL,
                          out_form=OUT_AFFINE, scalars_plain=plain)
                assert (got == want[:n]).all(), (value, plain)


def _edge_calls(engine, g, k, row, edge, others, vecs, plain_only=False):
    """one call per edge scalar, in row `row`; the other rows keep their scalars.  Returns the edge scalars that went wrong."""
    bad = []
    for e in edge:
        ks = others[:row] + [e] + others[row + 1:]
        want = g.expected(vecs, ks)
        for plain in ((True,) if plain_only else (False, True)):
            got = run(engine, g, vecs, g.plain(ks) if plain else g.mont(ks), base_form=SPECIAL, out_form=OUT_AFFINE,
                      scalars_plain=plain)
            if (got != want).any():
                bad.append((e if e < g.r - 100 else f"r + {e - g.r}", plain))
    return bad


ROWS = [pytest.param(k, row, id=f"k{k}-row{row}") for k in (2, 3) for row in range(k)]


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("k,row", ROWS)
def test_edge_scalars(engine, port, name, k, row):
    """Small scalars, powers of two, r - 2, r - 1 in both scalar forms, in row `row` beside random full-length scalars in
    the other rows.  Runs with the engine's default: the split for alt_bn128 G1, none for the others."""
    g, vecs, ks, _ = vector(port, name, k)
    assert not _edge_calls(engine, g, k, row, EDGE_SMALL + [g.r - 2, g.r - 1], ks, [v[5:6] for v in vecs])


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("k,row", ROWS)
def test_edge_scalars_around_r(engine, port, name, k, row):
    """As plain integers the sweep r - 40 .. r + 40 and the all-ones integer, whose top window carries out: a plain scalar
    >= r gives the multiple mod r."""
    g, vecs, ks, _ = vector(port, name, k)
    sweep = list(range(g.r - 40, g.r + 41)) + [(1 << (64 * g.fl)) - 1]
    assert not _edge_calls(engine, g, k, row, sweep, ks, [v[5:6] for v in vecs], plain_only=True)


@pytest.mark.parametrize("name", [p for p in ALL if not p.values[0].startswith("mnt")])
@pytest.mark.parametrize("k,row", ROWS)
def test_edge_scalars_with_the_split(engine, port, name, k, row):
    """the listed scalars again with the split asked for (the groups that have one), and the plain integers next to r and
    the all-ones one, which the split takes as they are"""
    g, vecs, ks, _ = vector(port, name, k)
    vecs = [v[9:10] for v in vecs]
    assert libff_amd.plan_fold(g.curve, g.group, k, 1, endomorphism=1)["endomorphism"]
    with endomorphism(engine, 1):
        assert not _edge_calls(engine, g, k, row, EDGE_SMALL + [g.r - 2, g.r - 1], ks, vecs)
        assert not _edge_calls(engine, g, k, row, [g.r - 1, g.r, g.r + 1, (1 << (64 * g.fl)) - 1], ks, vecs, plain_only=True)


@pytest.mark.parametrize("name", ALL)
def test_zero_scalars_and_rows_of_different_length(engine, port, name):
    """all k scalars zero: n zeros (no window holds a digit); a 64-bit scalar beside a full-length one, a 64-bit and a
    128-bit one alone: the ladder starts at the highest window any row uses"""
    g, vecs, ks, _ = vector(port, name, 3)
    n = 33
    vecs = [v[:n] for v in vecs]
    short, mid = ks[0] & ((1 << 64) - 1) | 1 << 63, ks[1] & ((1 << 128) - 1) | 1 << 127
    for value in (-1, 1):
        with endomorphism(engine, value):
            for k, scal in ((2, [0, 0]), (3, [0, 0, 0]), (2, [short, ks[1]]), (2, [ks[0], short]), (2, [short, mid]),
                            (3, [short, 0, 3]), (1, [short])):
                want = g.expected(vecs[:k], scal)
                if not any(scal):
                    assert (want == g.infinity()).all()
                for plain in (False, True):
                    got = run(engine, g, vecs[:k], g.plain(scal) if plain else g.mont(scal), base_form=SPECIAL,
                              out_form=OUT_AFFINE, scalars_plain=plain)
                    assert (got == want).all(), (value, scal, plain)


@pytest.mark.parametrize("name", ALL)
def test_edge_points(engine, port, name):
    """k = 2.  P_1 = P_0 with equal scalars (the equal-point branch at every window), P_1 = -P_0 with equal scalars (the
    opposite branch: zero), P_1 = P_0 with s_1 = r - s_0 (zero), P_1 = 2 P_0 with (2, r - 1) (zero), infinity in either
    vector and in both; each case also as a whole wave of 64 lanes that hold the same pair.  Both base forms."""
    g, vecs, ks, _ = vector(port, name, 2)
    s = ks[0]
    P, Q, inf = g.pool[3], g.pool[11], g.infinity()

    def layout(p0, p1):
        """the pair in every lane of the first wave, then once more among other pairs"""
        v0 = np.stack([p0] * 64 + [Q, P, p0, Q])
        v1 = np.stack([p1] * 64 + [P, Q, p1, P])
        return [v0, v1]

    cases = [(layout(P, P), [s, s], False), (layout(P, g.neg(P)), [s, s], True), (layout(P, P), [s, g.r - s], True),
             (layout(P, g.dbl(P)), [2, g.r - 1], True), (layout(inf, P), [s, ks[1]], False), (layout(P, inf), [s, ks[1]], False),
             (layout(inf, inf), [s, ks[1]], True), (layout(inf, P), [s, 0], True), (layout(inf, P), [0, s], False),
             (layout(P, inf), [0, s], True), (layout(inf, inf), [0, 0], True)]
    for pts, scal, zero in cases:
        want = g.expected(pts, scal)
        assert (want[0] == inf).all() == zero and (want[:64] == want[0]).all() and (want[66] == want[0]).all()
        for base_form in (SPECIAL, NORMAL):
            src = pts if base_form == SPECIAL else [g.scale(v, seed=12 + j) for j, v in enumerate(pts)]
            for out_form in (OUT_AFFINE, OUT_LIBFF):
                got = run(engine, g, src, g.mont(scal), base_form=base_form, out_form=out_form)
                assert (got == want).all(), (scal, base_form, out_form)


@pytest.mark.parametrize("name", ALL)
def test_aliased_inputs(engine, port, name):
    """the same array as P_0 and P_1: (s_0 + s_1) P; the two halves of one 128-element array: the inner-product fold"""
    g, vecs, ks, _ = vector(port, name, 2)
    v = np.ascontiguousarray(vecs[0][:64])
    got = run(engine, g, [v, v], g.mont(ks), base_form=SPECIAL, out_form=OUT_AFFINE)
    assert (got == g.expected([v], [ks[0] + ks[1]])).all()
    whole = np.ascontiguousarray(np.concatenate([vecs[0][:64], vecs[1][:64]]))
    lo, hi = whole[:64], whole[64:]
    assert hi.ctypes.data == whole.ctypes.data + 64 * g.gl * 8   # views of the one allocation, not copies
    x = ks[0]
    got = run(engine, g, [lo, hi], g.mont([pow(x, -1, g.r), x]), base_form=SPECIAL, out_form=OUT_AFFINE)
    assert (got == g.expected([lo, hi], [pow(x, -1, g.r), x])).all()


@pytest.mark.parametrize("name", ALL)
def test_cross_check_against_multi_exp(engine, port, name):
    """k = 3, n = 64: the sum of the outputs = multi_exp over the 192 inputs with each scalar repeated"""
    g, vecs, ks, _ = vector(port, name, 3)
    n = 64
    outs = engine.fold_vec(g.curve, g.group, [v[:n] for v in vecs], g.mont(ks), base_form=SPECIAL, out_form=OUT_LIBFF)
    lhs = engine.multi_exp(g.curve, g.group, outs, g.mont([1] * n), base_form=NORMAL, out_form=OUT_AFFINE)
    rhs = engine.multi_exp(g.curve, g.group, np.concatenate([v[:n] for v in vecs]), g.mont([k for k in ks for _ in range(n)]),
                           base_form=SPECIAL, out_form=OUT_AFFINE)
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
    """resident inputs made on the device by gen_bases_seq_device at three different `first` (windows of the pool),
    chunked and on a stream of the caller's"""
    g, _, ks, _ = vector(port, name, 3)
    n, step = g.distinct // 2, g.distinct // 4
    s = libff_amd.sizes(g.curve, g.group)
    d_vecs = [engine.malloc(n * s["affine_bytes"]) for _ in range(3)]
    d_out = engine.malloc(n * s["g_bytes"])
    try:
        for j, d in enumerate(d_vecs):
            engine.gen_bases_seq_device(g.curve, g.group, FIRST + j * step, n, d)
        # the same points as special-form records, for the expected values
        engine.export_affine_device(g.curve, g.group, d_vecs[1], n, d_out)
        engine.synchronize()
        pts = np.zeros((n, g.gl), dtype=np.uint64)
        engine.d2h(pts, d_out)
        assert (pts == g.pool[step:step + n]).all()
        want = g.expected([g.pool[j * step:j * step + n] for j in range(3)], ks)
        hip, stream = _hip_runtime(), ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        for out_form, chunk, st in ((OUT_AFFINE, 0, None), (OUT_LIBFF, 5, None), (OUT_AFFINE, n // 2 + 1, stream)):
            engine.fold_vec_device(g.curve, g.group, d_vecs, g.mont(ks), n, d_out, out_form=out_form, chunk_points=chunk, stream=st)
            if st is not None:
                assert hip.hipStreamSynchronize(st) == 0   # the call ran on the caller's stream: nothing else is waited for
            else:
                engine.synchronize()
            got = np.zeros((n, g.gl), dtype=np.uint64)
            engine.d2h(got, d_out)
            assert ((got if out_form == OUT_AFFINE else g.special(got)) == want).all(), (out_form, chunk)
        assert hip.hipStreamDestroy(stream) == 0
    finally:
        for p in d_vecs + [d_out]:
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_two_chained_rounds_on_the_device(engine, port, name):
    """fold 128 -> 64 with OUT_AFFINE, import_bases_device(form special), fold 64 -> 32: two rounds of an inner-product
    argument without the vector leaving the device"""
    g, _, ks, _ = vector(port, name, 2)
    s = libff_amd.sizes(g.curve, g.group)
    whole = g.pool[[(i + 5 * (i // 32)) % g.distinct for i in range(128)]]
    x, y = ks
    xi, yi = pow(x, -1, g.r), pow(y, -1, g.r)
    # G''[i] = yi (xi V[i] + x V[64 + i]) + y (xi V[32 + i] + x V[96 + i])
    want = g.expected([whole[0:32], whole[64:96], whole[32:64], whole[96:128]], [yi * xi, yi * x, y * xi, y * x])
    d_xyz, d_aff, d_out = engine.malloc(128 * s["g_bytes"]), engine.malloc(128 * s["affine_bytes"]), engine.malloc(64 * s["g_bytes"])
    try:
        engine.h2d(d_xyz, whole)
        engine.import_bases_device(g.curve, g.group, d_xyz, s["g_bytes"], SPECIAL, 128, d_aff)
        half = lambda p, n: ctypes.c_void_p(p.value + n * s["affine_bytes"])
        engine.fold_vec_device(g.curve, g.group, [d_aff, half(d_aff, 64)], g.mont([xi, x]), 64, d_out, out_form=OUT_AFFINE)
        engine.import_bases_device(g.curve, g.group, d_out, s["g_bytes"], SPECIAL, 64, d_aff)
        engine.fold_vec_device(g.curve, g.group, [d_aff, half(d_aff, 32)], g.mont([yi, y]), 32, d_out, out_form=OUT_AFFINE)
        engine.synchronize()
        got = np.zeros((32, g.gl), dtype=np.uint64)
        engine.d2h(got, d_out)
        assert (got == want).all()
    finally:
        for p in (d_xyz, d_aff, d_out):
            engine.free(p)


@pytest.mark.parametrize("name", ALL)
def test_refused_calls_leave_the_output_alone(engine, port, name):
    g, vecs, ks, want = vector(port, name, 2)
    n = 4
    sc = g.mont(ks)
    s = libff_amd.sizes(g.curve, g.group)
    out = np.full((n, g.gl), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    wide = [np.zeros((n, g.gl + 1), dtype=np.uint64) for _ in range(2)]
    for w, v in zip(wide, vecs):
        w[:, :g.gl] = v[:n]
    o = engine._opts(out_form=OUT_AFFINE)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    arr = lambda *ps: (ctypes.c_void_p * 9)(*ps)
    both = arr(ptr(wide[0]), ptr(wide[1]))
    nine = arr(*[ptr(wide[0])] * 9)
    call = lambda curve, group, k, pts, stride, scal, dst: engine.lib.amdmsm_fold_vec(
        engine.h, curve, group, k, pts, ctypes.c_size_t(stride), SPECIAL, scal, ctypes.c_size_t(n), dst, ctypes.c_size_t(0),
        ctypes.byref(o))
    nine_sc = g.mont(list(range(1, 10)))
    assert call(g.curve, g.group, 0, both, s["g_bytes"], ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, 9, nine, s["g_bytes"], ptr(nine_sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, 2, None, s["g_bytes"], ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, 2, arr(ptr(wide[0]), None), s["g_bytes"], ptr(sc), ptr(out)) == BAD_ARG
    assert b"vector 1" in engine.lib.amdmsm_last_error(engine.h)
    assert call(g.curve, g.group, 2, both, s["g_bytes"], None, ptr(out)) == BAD_ARG
    # a stride that is no multiple of the record alignment (4 bytes more than a record), one shorter than a record
    assert call(g.curve, g.group, 2, both, s["g_bytes"] + 4, ptr(sc), ptr(out)) == BAD_ARG
    assert call(g.curve, g.group, 2, both, s["g_bytes"] - 16, ptr(sc), ptr(out)) == BAD_ARG
    assert call(MNT6, G2, 2, both, s["g_bytes"], ptr(sc), ptr(out)) == UNSUPPORTED
    dev = lambda curve, group, k, pts, scal: engine.lib.amdmsm_fold_vec_device(
        engine.h, curve, group, k, pts, scal, ctypes.c_size_t(n), ptr(out), ctypes.c_size_t(0), ctypes.byref(o))
    assert dev(MNT6, G2, 2, both, ptr(sc)) == UNSUPPORTED
    assert dev(g.curve, g.group, 0, both, ptr(sc)) == BAD_ARG and dev(g.curve, g.group, 9, nine, ptr(nine_sc)) == BAD_ARG
    assert dev(g.curve, g.group, 2, None, ptr(sc)) == BAD_ARG and dev(g.curve, g.group, 2, both, None) == BAD_ARG
    assert dev(g.curve, g.group, 2, arr(None, ptr(wide[1])), ptr(sc)) == BAD_ARG
    assert b"vector 0" in engine.lib.amdmsm_last_error(engine.h)
    assert (out == 0x5a5a5a5a5a5a5a5a).all()
    # a padded stride that keeps the alignment is accepted
    padded = [np.concatenate([w, w], axis=1)[:, :2 * g.gl] for w in wide]
    got = engine.fold_vec(g.curve, g.group, padded, sc, base_form=SPECIAL, out_form=OUT_AFFINE, stride_bytes=2 * s["g_bytes"])
    assert (got == want[:n]).all()
