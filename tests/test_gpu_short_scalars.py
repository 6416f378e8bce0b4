"""amdmsm_multi_exp_short / amdmsm_msm_device_short / amdmsm_scalar_bits_device on the device: packed integers and Fr
records with a promised or measured bit length.  Every result against the CPU oracle's multi_exp on the scalars widened
to Fr (oracle.port for the pairing-curve groups; for the MNT groups the integer model of tests/mnt_model.py over a small
pool of points repeated along the vector, whose MSM is a closed form), and byte for byte against the engine's own
multi_exp on the widened scalars."""
import ctypes
import random

import numpy as np
import pytest

import mnt_model as mm
from common import GROUPS

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import G1, G2, MNT4, MNT6, OUT_AFFINE, multi_exp_base_form_special  # noqa: E402

BAD_ARG, UNSUPPORTED = -2, -3
MNT_GROUPS = [("mnt4_g1", MNT4, G1), ("mnt4_g2", MNT4, G2), ("mnt6_g1", MNT6, G1)]
MNT_MODELS = {"mnt4_g1": mm.MNT4, "mnt4_g2": mm.MNT4_G2, "mnt6_g1": mm.MNT6}
ALL_GROUPS = GROUPS + MNT_GROUPS
BY_NAME = {g[0]: g for g in ALL_GROUPS}
KINDS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SIZES = [1, 15, 16, 17, 63, 64, 65, 1000]
POOL = 24   # distinct points of an MNT base vector


class Backend:
    """bases, widened scalars and expected MSM values of one group; everything it hands out is cached and left unchanged"""

    def __init__(self, port, name):
        self.name, self.curve, self.group = BY_NAME[name]
        self.port = port
        self.model = MNT_MODELS.get(name)
        self.fl = libff_amd.sizes(self.curve, self.group)["fr_bytes"] // 8
        self._bases = {}
        if self.model:
            self.pool_pts = self.model.random_points(POOL, 5)
            self.pool = self.model.records(self.pool_pts)

    def bases(self, n):
        if n not in self._bases:
            if self.model:
                self._bases[n] = self.pool[np.arange(n) % POOL].copy()
            else:
                self._bases[n] = self.port.bases_seq(self.curve, self.group, n, first=3)
        return self._bases[n]

    def plain(self, ints):
        out = np.zeros((len(ints), self.fl), dtype=np.uint64)
        for i, k in enumerate(ints):
            for j in range(self.fl):
                out[i, j] = (int(k) >> (64 * j)) & ((1 << 64) - 1)
        return out

    def mont(self, ints):
        if self.model:
            return self.model.scalars_mont([int(k) for k in ints])
        return self.port.fr_from_bigint(self.curve, self.plain(ints))

    def want(self, n, ints):
        """the oracle's multi_exp of (bases(n), ints), canonical"""
        if self.model:
            sums = [0] * POOL
            for i, k in enumerate(ints):
                sums[i % POOL] += int(k)
            return self.model.msm(self.pool_pts, sums)
        if n == 0:
            return tuple(self.port.group_consts(self.curve, self.group)[1])
        return tuple(self.port.multi_exp(self.curve, self.group, self.bases(n), self.mont(ints), self.port.BDLO12_SIGNED, 1,
                                         chunks=8, omp=True))

    def canon(self, rec):
        if self.model:
            return self.model.point(rec)
        return tuple(self.port.group_op(self.curve, self.group, 4, rec))


_backends = {}


def backend(port, name):
    if name not in _backends:
        _backends[name] = Backend(port, name)
    return _backends[name]


class DeviceVectors:
    """compact affine bases of a group in HBM, an output record and a scalar buffer with room for an offset"""

    def __init__(self, engine, be, n_max):
        self.e, self.be = engine, be
        s = libff_amd.sizes(be.curve, be.group)
        self.g_bytes, self.aff_bytes = s["g_bytes"], s["affine_bytes"]
        self.n_max = max(n_max, 1)
        self.d_xyz = engine.malloc(self.n_max * self.g_bytes)
        self.d_aff = engine.malloc(self.n_max * self.aff_bytes)
        self.d_sc = engine.malloc(self.n_max * s["fr_bytes"] + 64)
        self.d_out = engine.malloc(self.g_bytes)
        self.loaded = None

    def load_bases(self, n):
        if self.loaded != n and n:
            self.e.h2d(self.d_xyz, self.be.bases(n))
            self.e.import_bases_device(self.be.curve, self.be.group, self.d_xyz, self.g_bytes, multi_exp_base_form_special, n,
                                       self.d_aff)
            self.loaded = n

    def scalars_at(self, arr, byte_offset):
        p = ctypes.c_void_p(self.d_sc.value + byte_offset)
        if arr.nbytes:
            self.e.h2d(p, arr)
        return p

    def raw(self, d_scalars, kind, n, bits, sentinel=None, **kw):
        """amdmsm_msm_device_short; returns (rc, output record)"""
        out = np.zeros(self.g_bytes // 8, dtype=np.uint64)
        if sentinel is not None:
            out[:] = sentinel
        self.e.h2d(self.d_out, out)
        o = self.e._opts(out_form=OUT_AFFINE, **kw)
        d = libff_amd.scalar_desc(kind, bits)
        rc = self.e.lib.amdmsm_msm_device_short(self.e.h, self.be.curve, self.be.group, self.d_aff, d_scalars, ctypes.byref(d),
                                                ctypes.c_size_t(n), self.d_out, ctypes.byref(o))
        self.e.synchronize()
        self.e.d2h(out, self.d_out)
        return rc, out

    def run(self, d_scalars, kind, n, bits, **kw):
        rc, out = self.raw(d_scalars, kind, n, bits, **kw)
        assert rc == 0, (rc, self.e.lib.amdmsm_last_error(self.e.h))
        return out

    def close(self):
        for p in (self.d_xyz, self.d_aff, self.d_sc, self.d_out):
            self.e.free(p)


@pytest.fixture
def dev(engine, port, request):
    made = []

    def make(name, n_max):
        d = DeviceVectors(engine, backend(port, name), n_max)
        made.append(d)
        return d

    yield make
    for d in made:
        d.close()


def values(kind, n, pattern, seed):
    dt = KINDS[kind]
    if pattern == "ones":
        return np.full(n, np.iinfo(dt).max, dtype=dt)
    if pattern == "zero":
        return np.zeros(n, dtype=dt)
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)


@pytest.mark.parametrize("kind", [1, 2, 4, 8], ids=["u8", "u16", "u32", "u64"])
@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_377_g2", "mnt4_g1"])
def test_widths_and_tails(engine, port, dev, name, kind):
    """every kind at lengths around the 16-byte vector (1, 15, 16, 17, 63, 64, 65, 1000), the device pointer on a 16-byte
    boundary and one element past it; random, all-0xFF and all-zero vectors; device entry, host entry and multi_exp on
    the widened scalars agree with the oracle"""
    be = backend(port, name)
    d = dev(name, max(SIZES))
    for n in SIZES:
        d.load_bases(n)
        for pattern in ("random", "ones", "zero"):
            v = values(kind, n, pattern, 100 * kind + n)
            want = be.want(n, v)
            wide = engine.multi_exp(be.curve, be.group, be.bases(n), be.mont(v), base_form=multi_exp_base_form_special)
            assert be.canon(wide) == want
            for off in (0, kind):
                got = d.run(d.scalars_at(v, off), kind, n, 0)
                assert (got == wide).all(), (n, pattern, off)
            if pattern == "random":
                got = engine.multi_exp_short(be.curve, be.group, be.bases(n), v, base_form=multi_exp_base_form_special)
                assert (got == wide).all(), (n, "host")
                assert engine.scalar_bits(be.curve, be.group, d.scalars_at(v, kind), kind, n) == int(max(v)).bit_length()


@pytest.mark.parametrize("name", [g[0] for g in ALL_GROUPS])
def test_every_group_u32(engine, port, dev, name):
    """U32, n = 1000, device and host entry, every group"""
    be = backend(port, name)
    n = 1000
    v = values(4, n, "random", 7)
    want = be.want(n, v)
    d = dev(name, n)
    d.load_bases(n)
    got_dev = d.run(d.scalars_at(v, 0), 4, n, 0)
    got_host = engine.multi_exp_short(be.curve, be.group, be.bases(n), v, base_form=multi_exp_base_form_special)
    wide = engine.multi_exp(be.curve, be.group, be.bases(n), be.mont(v), base_form=multi_exp_base_form_special)
    assert be.canon(got_dev) == want and be.canon(got_host) == want
    assert (got_dev == wide).all() and (got_host == wide).all()


@pytest.mark.parametrize("plain", [False, True], ids=["mont", "plain"])
@pytest.mark.parametrize("c", [4, 13, 16])
@pytest.mark.parametrize("name", ["alt_bn128_g1", "mnt6_g1"])
def test_window_boundaries(engine, port, dev, name, c, plain):
    """Fr records with a promised length of c - 2, c - 1, c, 2c - 2, 2c - 1 bits (1, 2 and 3 windows), the extreme scalars
    2^bits - 1 and 2^(bits - 1) several times each (equal digits: buckets that span lanes); the same with the length
    measured, which must be the true maximum"""
    be = backend(port, name)
    n = 257
    d = dev(name, n)
    d.load_bases(n)
    windows = set()
    for bits in (c - 2, c - 1, c, 2 * c - 2, 2 * c - 1):
        rng = random.Random(1000 * c + bits)
        ints = [rng.randrange(1 << bits) for _ in range(n)]
        for i in range(0, 40, 2):
            ints[i] = (1 << bits) - 1
            ints[i + 1] = 1 << (bits - 1)
        ints[n - 1] = (1 << bits) - 1
        longest = max(ints).bit_length()
        assert longest == bits
        want = be.want(n, ints)
        sc = be.plain(ints) if plain else be.mont(ints)
        wide = engine.multi_exp(be.curve, be.group, be.bases(n), sc, base_form=multi_exp_base_form_special, scalars_plain=plain,
                                window_bits=c)
        assert be.canon(wide) == want
        p = libff_amd.plan_short(be.curve, be.group, n, bits, window_bits=c)
        assert p["num_windows"] == (bits + 2 + c - 1) // c and not p["endomorphism"]
        windows.add(p["num_windows"])
        d_sc = d.scalars_at(sc, 0)
        for b in (bits, -1):
            got = d.run(d_sc, 0, n, b, window_bits=c, scalars_plain=plain)
            assert (got == wide).all(), (bits, b, "device")
            got = engine.multi_exp_short(be.curve, be.group, be.bases(n), sc, bits=b, base_form=multi_exp_base_form_special,
                                         window_bits=c, scalars_plain=plain)
            assert (got == wide).all(), (bits, b, "host")
        assert engine.scalar_bits(be.curve, be.group, d_sc, 0, n, scalars_plain=plain) == longest
    assert windows == {1, 2, 3}


@pytest.mark.parametrize("n", [(1 << 14) + 3, 1 << 16])
@pytest.mark.parametrize("what", ["u32", "fr64"])
def test_larger_sizes(engine, port, dev, what, n):
    """the planner's own window size over the two-level sort: U32, and Fr records promised to be below 2^64"""
    be = backend(port, "alt_bn128_g1")
    d = dev("alt_bn128_g1", n)
    d.load_bases(n)
    rng = np.random.default_rng(n)
    if what == "u32":
        v = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        kind, bits, sc = 4, 0, v
    else:
        v = rng.integers(0, np.iinfo(np.uint64).max, size=n, dtype=np.uint64, endpoint=True)
        kind, bits, sc = 0, 64, be.mont(v)
    p = libff_amd.plan_short(be.curve, be.group, n, 32 if what == "u32" else 64)
    assert 1 <= p["num_windows"] <= 34 and not p["endomorphism"]
    want = be.want(n, v)
    wide = engine.multi_exp(be.curve, be.group, be.bases(n), be.mont(v), base_form=multi_exp_base_form_special)
    assert be.canon(wide) == want
    got = d.run(d.scalars_at(sc, 0), kind, n, bits)
    assert (got == wide).all()
    got = engine.multi_exp_short(be.curve, be.group, be.bases(n), sc, bits=bits, base_form=multi_exp_base_form_special)
    assert (got == wide).all()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_broken_promise(engine, port, dev, where):
    """bits = 32 with exactly one scalar equal to 2^32: both entries refuse, the output keeps its sentinel, and the next
    ordinary call on the context is correct"""
    be = backend(port, "alt_bn128_g1")
    n = 300
    d = dev("alt_bn128_g1", n)
    d.load_bases(n)
    rng = random.Random(3)
    ints = [rng.randrange(1 << 32) for _ in range(n)]
    good, good_ints = be.mont(ints), list(ints)
    ints[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = 1 << 32
    bad = be.mont(ints)
    sentinel = 0x5A5A5A5A5A5A5A5A
    rc, out = d.raw(d.scalars_at(bad, 0), 0, n, 32, sentinel=sentinel)
    assert rc == BAD_ARG and (out == sentinel).all()
    host_out = np.full(d.g_bytes // 8, sentinel, dtype=np.uint64)
    o = engine._opts(out_form=OUT_AFFINE)
    desc = libff_amd.scalar_desc(0, 32)
    bases = be.bases(n)
    rc = engine.lib.amdmsm_multi_exp_short(engine.h, be.curve, be.group, bases.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_size_t(d.g_bytes), 1, bad.ctypes.data_as(ctypes.c_void_p), ctypes.byref(desc),
                                           ctypes.c_size_t(n), host_out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(o))
    assert rc == BAD_ARG and (host_out == sentinel).all()
    # packed integers with a promise below their width are tested in the same way
    v = np.array([1, 2, 1 << 16, 3], dtype=np.uint32)
    d.load_bases(n)
    rc, out = d.raw(d.scalars_at(v, 0), 4, 4, 16, sentinel=sentinel)
    assert rc == BAD_ARG and (out == sentinel).all()
    # the context is as good as before
    want = be.want(n, good_ints)
    got = engine.multi_exp(be.curve, be.group, bases, good, base_form=multi_exp_base_form_special)
    assert be.canon(got) == want
    got_short = d.run(d.scalars_at(good, 0), 0, n, 32)
    assert (got_short == got).all()


def test_refusals_before_launch(engine, port, dev):
    be = backend(port, "alt_bn128_g1")
    n = 8
    d = dev("alt_bn128_g1", n)
    d.load_bases(n)
    v = np.arange(n, dtype=np.uint32)
    d_sc = d.scalars_at(v, 0)
    sentinel = 0x1111111111111111

    def call(kind=4, bits=0, struct_size=None, curve=be.curve, group=be.group, window_bits=0):
        out = np.full(d.g_bytes // 8, sentinel, dtype=np.uint64)
        engine.h2d(d.d_out, out)
        o = engine._opts(out_form=OUT_AFFINE, window_bits=window_bits)
        desc = libff_amd.scalar_desc(kind, bits)
        if struct_size is not None:
            desc.struct_size = struct_size
        rc = engine.lib.amdmsm_msm_device_short(engine.h, curve, group, d.d_aff, d_sc, ctypes.byref(desc), ctypes.c_size_t(n),
                                                d.d_out, ctypes.byref(o))
        engine.synchronize()
        engine.d2h(out, d.d_out)
        assert (out == sentinel).all()
        host = np.full(d.g_bytes // 8, sentinel, dtype=np.uint64)
        bases = be.bases(n)
        rc_h = engine.lib.amdmsm_multi_exp_short(engine.h, curve, group, bases.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_size_t(d.g_bytes), 1, v.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.byref(desc), ctypes.c_size_t(n), host.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.byref(o))
        assert (host == sentinel).all()
        return rc, rc_h

    assert call(struct_size=8) == (BAD_ARG, BAD_ARG)
    assert call(struct_size=16) == (BAD_ARG, BAD_ARG)
    assert call(kind=3) == (BAD_ARG, BAD_ARG)
    assert call(kind=16) == (BAD_ARG, BAD_ARG)
    assert call(bits=-2) == (BAD_ARG, BAD_ARG)
    assert call(bits=33) == (BAD_ARG, BAD_ARG)                     # above the kind's width
    assert call(kind=0, bits=255) == (BAD_ARG, BAD_ARG)            # alt_bn128 Fr has 254 bits
    assert call(window_bits=23) == (BAD_ARG, BAD_ARG)
    assert call(curve=MNT6, group=G2) == (UNSUPPORTED, UNSUPPORTED)
    bits = ctypes.c_int(-5)
    desc = libff_amd.scalar_desc(3, 0)
    assert engine.lib.amdmsm_scalar_bits_device(engine.h, be.curve, be.group, d_sc, ctypes.c_size_t(n), ctypes.byref(desc), 0,
                                                ctypes.byref(bits)) == BAD_ARG


def test_edge_results(engine, port, dev):
    """n = 0 gives zero; all-zero scalars with the length measured give zero (and measure 0)"""
    be = backend(port, "alt_bn128_g1")
    zero = tuple(port.group_consts(be.curve, be.group)[1])
    n = 100
    d = dev("alt_bn128_g1", n)
    d.load_bases(n)
    for kind in (0, 4):
        assert tuple(d.run(None, kind, 0, 0, sentinel=7)) == zero
        assert tuple(d.run(None, kind, 0, -1, sentinel=7)) == zero
        sc = np.zeros((n, be.fl), dtype=np.uint64) if kind == 0 else np.zeros(n, dtype=np.uint32)
        d_sc = d.scalars_at(sc, 0)
        assert engine.scalar_bits(be.curve, be.group, d_sc, kind, n) == 0
        assert tuple(d.run(d_sc, kind, n, -1, sentinel=7)) == zero
        got = engine.multi_exp_short(be.curve, be.group, be.bases(n), sc, bits=-1, base_form=multi_exp_base_form_special)
        assert tuple(got) == zero
    no_bases = np.zeros((0, d.g_bytes // 8), dtype=np.uint64)
    got = engine.multi_exp_short(be.curve, be.group, no_bases, np.zeros(0, dtype=np.uint16))
    assert tuple(got) == zero


def test_registered_bases(engine, port):
    """the host entry reads a registered base vector's resident copy: same bytes as without registration"""
    be = backend(port, "bls12_377_g1")
    n = 600
    bases = be.bases(n).copy()
    v = values(2, n, "random", 9)
    before = engine.multi_exp_short(be.curve, be.group, bases, v, base_form=multi_exp_base_form_special)
    assert be.canon(before) == be.want(n, v)
    h = engine.register_bases(be.curve, be.group, bases, base_form=multi_exp_base_form_special)
    try:
        after = engine.multi_exp_short(be.curve, be.group, bases, v, base_form=multi_exp_base_form_special)
        part = engine.multi_exp_short(be.curve, be.group, bases[100:500], v[100:500], base_form=multi_exp_base_form_special)
    finally:
        engine.unregister_bases(h)
    assert (after == before).all()
    assert (part == engine.multi_exp_short(be.curve, be.group, bases[100:500].copy(), v[100:500].copy(),
                                           base_form=multi_exp_base_form_special)).all()
