"""amdmsm_multi_exp_batch_items / amdmsm_msm_device_batch_items: MSMs of different lengths in one batch, their scalars
own vectors, slices of one shared vector or index lists into it.  Every result against the oracle's MSM of the
materialised (bases, selected scalars): the C restatement (oracle.port) for the pairing-curve groups, the integer model
(tests/mnt_model.py) for the MNT groups, closed forms at full size."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mnt_model as mm
from common import GROUPS, golden, to_int

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G1, G2, MNT4, MNT6, OUT_AFFINE, OUT_LIBFF, BatchItem, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special)
from libff_amd.engine import BatchItemStruct  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -2, -3
MNT_GROUPS = [("mnt4_g1", MNT4, G1), ("mnt4_g2", MNT4, G2), ("mnt6_g1", MNT6, G1)]
MNT_MODELS = {"mnt4_g1": mm.MNT4, "mnt4_g2": mm.MNT4_G2, "mnt6_g1": mm.MNT6}
ALL_GROUPS = GROUPS + MNT_GROUPS


class PortBackend:
    """inputs and expected values of a pairing-curve group from oracle.port"""

    def __init__(self, port, curve, group):
        self.port, self.curve, self.group = port, curve, group
        self.zero = tuple(port.group_consts(curve, group)[1])

    def bases(self, n, seed):
        return self.port.bases_seq(self.curve, self.group, n, first=seed)

    def normal_form(self, bases):
        """other points in genuinely projective records: every third one becomes 3 P with Z != 1"""
        p, out = self.port, bases.copy()
        for i in range(0, len(bases), 3):
            out[i] = p.group_op(self.curve, self.group, 0, p.group_op(self.curve, self.group, 2, bases[i]), bases[i])
        return out

    def scalars(self, n, seed):
        return self.port.scalars_sha512(self.curve, seed, n)

    def small_scalar(self, v):
        plain = np.zeros((1, libff_amd.sizes(self.curve, self.group)["fr_bytes"] // 8), dtype=np.uint64)
        plain[0, 0] = v
        return self.port.fr_from_bigint(self.curve, plain)[0]

    def plain(self, sc):
        return self.port.fr_as_bigint(self.curve, sc)

    def neg(self, rec):
        return self.port.group_op(self.curve, self.group, 3, rec)

    def msm(self, bases, sc, special=True):
        if len(bases) == 0:
            return self.zero
        return tuple(self.port.multi_exp(self.curve, self.group, bases, sc, self.port.BDLO12_SIGNED, 1 if special else 0,
                                         chunks=8, omp=True))

    def canon(self, rec):
        return tuple(self.port.group_op(self.curve, self.group, 4, rec))


class MntBackend:
    """the same from the integer model of the MNT curves"""

    def __init__(self, model, curve, group):
        self.model, self.curve, self.group = model, curve, group
        self.zero = mm.INF
        self.rinv = pow(mm.RADIX, -1, model.r)

    def bases(self, n, seed):
        return self.model.records(self.model.random_points(n, seed))

    def normal_form(self, bases):
        rng = random.Random(len(bases))
        pts = [self.model.point(r) for r in bases]
        return self.model.records(pts, [rng.randrange(1, self.model.p) for _ in pts])

    def scalars(self, n, seed):
        rng = random.Random(seed)
        return self.model.scalars_mont([rng.randrange(self.model.r) for _ in range(n)])

    def small_scalar(self, v):
        return self.model.scalars_mont([v])[0]

    def ints(self, sc):
        return [mm.to_int(row) * self.rinv % self.model.r for row in sc]

    def plain(self, sc):
        return np.array([mm.words(k) for k in self.ints(sc)], dtype=np.uint64).reshape(len(sc), mm.WORDS)

    def neg(self, rec):
        return self.model.records([self.model.neg(self.model.point(rec))])[0]

    def msm(self, bases, sc, special=True):
        return self.model.msm([self.model.point(r) for r in bases], self.ints(sc))

    def canon(self, rec):
        return self.model.point(rec)


def backend(port, name, curve, group):
    return MntBackend(MNT_MODELS[name], curve, group) if name in MNT_MODELS else PortBackend(port, curve, group)


def materialise(it, shared):
    """the scalar vector an item selects"""
    n = len(it.bases)
    if it.scalars is not None:
        return it.scalars
    if it.index is not None:
        return shared[np.asarray(it.index, dtype=np.int64)]
    return shared[it.offset:it.offset + n]


def check_batch(engine, be, items, shared, special=True, **kw):
    want = [be.msm(it.bases, materialise(it, shared), special) for it in items]
    form = multi_exp_base_form_special if special else multi_exp_base_form_normal
    got = engine.multi_exp_batch_items(be.curve, be.group, items, shared, base_form=form, **kw)
    for j, (g, w) in enumerate(zip(got, want)):
        assert be.canon(g) == w, (j, kw)
    return got


def four_items(be, shared_n=400):
    """lengths (257, 64, 1, 300): the prefix, a slice at an offset, an index list with repeats in descending order, an own vector"""
    shared = be.scalars(shared_n, 7)
    idx = np.array([399], dtype=np.uint32)
    items = [BatchItem(be.bases(257, 1)), BatchItem(be.bases(64, 2), offset=123), BatchItem(be.bases(1, 3), index=idx),
             BatchItem(be.bases(300, 4), scalars=be.scalars(300, 8))]
    return items, shared


@pytest.mark.parametrize("name,curve,group", ALL_GROUPS)
def test_every_group_both_forms(engine, port, name, curve, group):
    """k = 4 items of lengths (257, 64, 1, 300) over 400 shared scalars: the prefix, 64 indices in descending order with
    repeats, a slice of one element at offset 123, an own vector; both base forms, Montgomery and plain scalars, both
    output forms."""
    be = backend(port, name, curve, group)
    items, shared = four_items(be)
    idx = np.array(sorted([5, 5, 399, 0, 17, 17, 17, 200] * 8, reverse=True), dtype=np.uint32)
    items[1] = BatchItem(items[1].bases, index=idx)
    items[2] = BatchItem(items[2].bases, offset=123)
    want = [be.msm(it.bases, materialise(it, shared)) for it in items]
    got_special = None
    for special in (True, False):
        its = items if special else [BatchItem(be.normal_form(it.bases), it.scalars, it.offset, it.index) for it in items]
        w = want if special else [be.msm(it.bases, materialise(it, shared), False) for it in its]
        form = multi_exp_base_form_special if special else multi_exp_base_form_normal
        for plain in (False, True):
            sh = be.plain(shared) if plain else shared
            its_p = [BatchItem(it.bases, None if it.scalars is None else (be.plain(it.scalars) if plain else it.scalars),
                               it.offset, it.index) for it in its]
            for out_form in (OUT_LIBFF, OUT_AFFINE):
                got = engine.multi_exp_batch_items(curve, group, its_p, sh, base_form=form, out_form=out_form,
                                                   scalars_plain=plain)
                assert [be.canon(g) for g in got] == w, (special, plain, out_form)
                if special and not plain and out_form == OUT_AFFINE:
                    got_special = got
    # in addition: the engine's own multi_exp on the materialised inputs gives the same records
    for it, g in zip(items, got_special):
        one = engine.multi_exp(curve, group, it.bases, materialise(it, shared), base_form=multi_exp_base_form_special)
        assert (one == g).all()


LENGTH_BATCHES = [
    [4097], [0], [1, 0], [0, 0, 7], [2, 7, 8], [255, 256, 257, 0], [0, 0, 0, 0, 0, 0, 0, 300],
    [1 << 16, 1, 1, 1, 1, 1, 1, 1], [8, 0, 4097, 1, 256, 2], [7, 255, 0, 1, 2, 257, 8],
]


@pytest.mark.parametrize("lengths", LENGTH_BATCHES, ids=lambda v: "-".join(map(str, v)))
def test_lengths(engine, port, lengths):
    """k = 1 .. 8 with lengths from {0, 1, 2, 7, 8, 255, 256, 257, 4097, 2^16}; items alternate between slice, index list
    and own vector; an empty item gives the group's zero in both output forms."""
    curve, group = 0, 1
    be = PortBackend(port, curve, group)
    n_max = max(max(lengths), 1)
    shared = be.scalars(n_max + 5, 11)
    pool = be.bases(n_max, 3)
    rng = np.random.default_rng(len(lengths))
    items = []
    for j, n in enumerate(lengths):
        b = pool[:n]
        if j % 3 == 0:
            items.append(BatchItem(b, offset=5 if n else 0))
        elif j % 3 == 1:
            items.append(BatchItem(b, index=rng.integers(0, len(shared), size=n).astype(np.uint32)))
        else:
            items.append(BatchItem(b, scalars=be.scalars(n, 20 + j)))
    for out_form in (OUT_AFFINE, OUT_LIBFF):
        got = check_batch(engine, be, items, shared, out_form=out_form)
        for n, g in zip(lengths, got):
            if n == 0:
                assert be.canon(g) == be.zero
                if out_form == OUT_AFFINE:
                    assert (g == port.group_consts(curve, group)[1]).all()   # the special form of zero, (0, 1, 0)
    for name, c, g_ in MNT_GROUPS[:1]:
        mb = backend(port, name, c, g_)
        got = engine.multi_exp_batch_items(c, g_, [BatchItem(mb.bases(0, 1)), BatchItem(mb.bases(2, 2))], mb.scalars(4, 1))
        assert mb.canon(got[0]) == mm.INF


@pytest.mark.parametrize("name,curve,group", [GROUPS[0], GROUPS[2], GROUPS[3]] + MNT_GROUPS[:1])
def test_endomorphism_on_and_off(engine, port, name, curve, group):
    """the same ragged batch with odd lengths, split forced and forbidden: identical group elements (MNT: option ignored)"""
    be = backend(port, name, curve, group)
    shared = be.scalars(700, 5)
    idx = np.arange(0, 699, 3, dtype=np.uint32)[::-1].copy()
    items = [BatchItem(be.bases(699, 1)), BatchItem(be.bases(len(idx), 2), index=idx), BatchItem(be.bases(1, 3), offset=698),
             BatchItem(be.bases(33, 4), scalars=be.scalars(33, 6))]
    saved, results = engine.endomorphism, []
    try:
        for endo in (-1, 2):
            engine.endomorphism = endo
            results.append(check_batch(engine, be, items, shared))
    finally:
        engine.endomorphism = saved
    for a, b in zip(*results):
        assert (a == b).all()


@pytest.mark.parametrize("name,curve,group", [GROUPS[0], GROUPS[2], MNT_GROUPS[0]])
def test_window_bits(engine, port, name, curve, group):
    """forced window sizes on a ragged batch; window_bits = 23 is AMDMSM_ERR_BAD_ARG, as for amdmsm_multi_exp_batch
    (the batch has no two-pass sort for c > 22)"""
    be = backend(port, name, curve, group)
    items, shared = four_items(be)
    for c in (2, 5, 13, 16, 22):
        check_batch(engine, be, items, shared, window_bits=c)
    with pytest.raises(libff_amd.AmdMsmError, match="bad argument"):
        engine.multi_exp_batch_items(curve, group, items, shared, window_bits=23)


@pytest.mark.parametrize("name,curve,group", [GROUPS[0], GROUPS[1], MNT_GROUPS[0], MNT_GROUPS[1]])
def test_special_cases_through_the_index_list(engine, port, name, curve, group):
    """all indices equal (every base meets the same scalar; repeated bases then double inside a bucket), and P beside -P
    with one scalar in one bucket"""
    be = backend(port, name, curve, group)
    shared = be.scalars(50, 9)
    shared[10] = be.small_scalar(37)    # one digit: every entry in one bucket of window 0
    n = 96
    b = be.bases(n, 2)
    same = np.repeat(b[:1], n, axis=0)
    pm = b.copy()
    pm[1::2] = be.neg(b[0])
    pm[0::2] = b[0]
    pm[n - 1] = b[5]                    # ... and one survivor
    for idx_val in (10, 33):
        idx = np.full(n, idx_val, dtype=np.uint32)
        items = [BatchItem(b, index=idx), BatchItem(same, index=idx), BatchItem(pm, index=idx)]
        for c in (0, 7):
            check_batch(engine, be, items, shared, window_bits=c)


def _raw_call(engine, curve, group, k, arr, shared, shared_n, stride):
    o = engine._opts(out_form=OUT_AFFINE)
    return engine.lib.amdmsm_multi_exp_batch_items(engine.h, curve, group, k, arr, ctypes.c_size_t(stride), 1,
                                                   shared.ctypes.data_as(ctypes.c_void_p) if shared is not None else None,
                                                   ctypes.c_size_t(shared_n), ctypes.byref(o))


def test_validation_leaves_outputs_untouched(engine, port):
    curve, group = 0, 1
    be = PortBackend(port, curve, group)
    s = libff_amd.sizes(curve, group)
    shared = be.scalars(100, 1)
    b = be.bases(40, 1)
    own = be.scalars(40, 2)
    idx_ok = np.arange(40, dtype=np.uint32)
    idx_bad = idx_ok.copy()
    idx_bad[17] = 100
    outs = np.full((2, s["g_bytes"] // 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    size = ctypes.sizeof(BatchItemStruct)

    def item(j, scalars=None, offset=0, index=None, struct_size=size):
        return BatchItemStruct(struct_size, vp(b), 40, None if scalars is None else vp(scalars), offset,
                               None if index is None else vp(index), vp(outs[j]))

    good = item(0, offset=3)
    cases = {
        "slice past shared_n": ([good, item(1, offset=61)], shared, 2),
        "index >= shared_n": ([good, item(1, index=idx_bad)], shared, 2),
        "scalars and index": ([good, item(1, scalars=own, index=idx_ok)], shared, 2),
        "no shared vector": ([item(0, scalars=own), item(1, offset=0)], None, 2),
        "struct_size": ([good, item(1, offset=0, struct_size=size - 8)], shared, 2),
        "k = 0": ([good, good], shared, 0),
        "k = 9": ([good] * 9, shared, 9),
        "stride": ([good, item(1)], shared, 2),
    }
    for what, (lst, sh, k) in cases.items():
        arr = (BatchItemStruct * len(lst))(*lst)
        stride = s["g_bytes"] + (4 if what == "stride" else 0)
        rc = _raw_call(engine, curve, group, k, arr, sh, 0 if sh is None else len(sh), stride)
        assert rc == BAD_ARG, what
        assert (outs == 0xA5A5A5A5A5A5A5A5).all(), what
    # the same items, valid: the call works after the refusals
    arr = (BatchItemStruct * 2)(good, item(1, index=idx_ok))
    assert _raw_call(engine, curve, group, 2, arr, shared, 100, s["g_bytes"]) == 0
    assert tuple(outs[0]) == be.msm(b, shared[3:43]) and tuple(outs[1]) == be.msm(b, shared[:40])
    o = engine._opts()
    assert engine.lib.amdmsm_multi_exp_batch_items(engine.h, MNT6, G2, 2, arr, ctypes.c_size_t(0), 1, vp(shared),
                                                   ctypes.c_size_t(100), ctypes.byref(o)) == UNSUPPORTED


class _Dev:
    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.eng.malloc(max(arr.nbytes, 8))
        self.ptrs.append(p)
        if arr.nbytes:
            self.eng.h2d(p, arr)
        return p.value

    def free(self):
        for p in self.ptrs:
            self.eng.free(p)


@pytest.mark.parametrize("name,curve,group", [GROUPS[0], GROUPS[3], MNT_GROUPS[2]])
def test_device_entry_and_index_guard(engine, port, name, curve, group):
    """the device entry on a ragged batch; then one index out of range among 4096: AMDMSM_ERR_BAD_ARG naming the item,
    nothing read past the shared vector (the guard takes scalar 0), and an ordinary multi_exp afterwards is correct"""
    be = backend(port, name, curve, group)
    s = libff_amd.sizes(curve, group)
    aw = s["affine_bytes"] // 8
    n = 4096 if name not in MNT_MODELS else 512
    shared = be.scalars(600, 3)
    b = be.bases(n, 1)
    idx = np.random.default_rng(1).integers(0, 600, size=n).astype(np.uint32)
    own = be.scalars(100, 4)
    dev = _Dev(engine)
    try:
        d_b, d_sh = dev.put(b[:, :aw]), dev.put(shared)
        d_idx, d_own = dev.put(idx), dev.put(own)
        d_out = [dev.put(np.zeros(s["g_bytes"] // 8, dtype=np.uint64)) for _ in range(4)]
        items = [dict(bases=d_b, n=n, index=d_idx, out=d_out[0]), dict(bases=d_b, n=500, offset=100, out=d_out[1]),
                 dict(bases=d_b, n=100, scalars=d_own, out=d_out[2]), dict(bases=None, n=0, out=d_out[3])]
        engine.msm_device_batch_items(curve, group, items, d_sh, 600, out_form=OUT_AFFINE)
        engine.synchronize()
        want = [be.msm(b, shared[idx.astype(np.int64)]), be.msm(b[:500], shared[100:600]), be.msm(b[:100], own), be.zero]
        for j in range(4):
            out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
            engine.d2h(out, ctypes.c_void_p(d_out[j]))
            assert be.canon(out) == want[j], j
        with pytest.raises(libff_amd.AmdMsmError, match="bad argument"):
            engine.msm_device_batch_items(curve, group, [dict(bases=d_b, n=500, offset=101, out=d_out[1])], d_sh, 600)
        bad = idx.copy()
        bad[n // 2] = 600
        engine.h2d(ctypes.c_void_p(d_idx), bad)
        with pytest.raises(libff_amd.AmdMsmError, match="item 1"):
            engine.msm_device_batch_items(curve, group, [items[1], items[0]], d_sh, 600, out_form=OUT_AFFINE)
        got = engine.multi_exp(curve, group, b, shared[idx.astype(np.int64)], base_form=multi_exp_base_form_special)
        assert be.canon(got) == want[0]
    finally:
        dev.free()


def test_registered_bases_and_equal_length_batch_around_a_ragged_call(engine, port):
    """two of four base vectors registered, the batch run twice: equal and correct.  The equal-length batch with the same
    inputs before and after the ragged calls gives identical records (the workspace is reused across plans of other shapes)."""
    curve, group = 0, 1
    be = PortBackend(port, curve, group)
    n = 3001
    eq_b = [be.bases(n, 50 * j) for j in range(3)]
    eq_s = [be.scalars(n, 70 + j) for j in range(3)]
    before = engine.multi_exp_batch(curve, group, eq_b, eq_s, base_form=multi_exp_base_form_special)
    shared = be.scalars(9000, 12)
    lens = (9000, 4097, 8000, 130)
    vecs = [be.bases(m, 1000 * (j + 1)) for j, m in enumerate(lens)]
    idx = np.sort(np.random.default_rng(2).choice(9000, size=4097, replace=False)).astype(np.uint32)
    items = [BatchItem(vecs[0]), BatchItem(vecs[1], index=idx), BatchItem(vecs[2], offset=1000),
             BatchItem(vecs[3], scalars=be.scalars(130, 13))]
    handles = [engine.register_bases(curve, group, vecs[j], multi_exp_base_form_special) for j in (0, 2)]
    try:
        first = check_batch(engine, be, items, shared)
        second = check_batch(engine, be, items, shared)
        for a, b in zip(first, second):
            assert (a == b).all()
    finally:
        for h in handles:
            engine.unregister_bases(h)
    after = engine.multi_exp_batch(curve, group, eq_b, eq_s, base_form=multi_exp_base_form_special)
    for j in range(3):
        assert (before[j] == after[j]).all() and tuple(after[j]) == be.msm(eq_b[j], eq_s[j])


@pytest.mark.parametrize("window_bits", [7, 12], ids=["segment-kernels", "row-column-sums"])
@pytest.mark.parametrize("name,curve,group", [GROUPS[0], GROUPS[3], MNT_GROUPS[0]])
def test_equal_length_and_ragged_entries_agree(engine, port, name, curve, group, window_bits):
    """k = 3 MSMs of 300 points through amdmsm_msm_device_batch and, every item with its own scalars, through
    amdmsm_msm_device_batch_items: the same records from both, equal to the oracle's; then the ragged call with one item
    of length 0 and one of length 1.  window_bits 7 takes the segment kernels, 12 the row / column sums."""
    be = backend(port, name, curve, group)
    s = libff_amd.sizes(curve, group)
    aw, gw = s["affine_bytes"] // 8, s["g_bytes"] // 8
    k, n = 3, 300
    bases = [be.bases(n, 10 * j + 1) for j in range(k)]
    scs = [be.scalars(n, 30 + j) for j in range(k)]
    exact = isinstance(be, PortBackend)   # the C restatement gives the record itself, the integer model the point

    def same(out, want):
        return tuple(out) == want if exact else be.canon(out) == want

    dev = _Dev(engine)
    try:
        d_b = [dev.put(b[:, :aw]) for b in bases]
        d_s = [dev.put(x) for x in scs]
        d_o = [dev.put(np.zeros(gw, dtype=np.uint64)) for _ in range(k)]

        def fetch():
            engine.synchronize()
            outs = np.zeros((k, gw), dtype=np.uint64)
            for j in range(k):
                engine.d2h(outs[j], ctypes.c_void_p(d_o[j]))
                engine.h2d(ctypes.c_void_p(d_o[j]), np.zeros(gw, dtype=np.uint64))
            return outs

        engine.msm_device_batch(curve, group, d_b, d_s, n, d_o, out_form=OUT_AFFINE, window_bits=window_bits)
        equal = fetch()
        lens = [n] * k
        items = lambda: [dict(bases=d_b[j], n=lens[j], scalars=d_s[j], out=d_o[j]) for j in range(k)]
        engine.msm_device_batch_items(curve, group, items(), out_form=OUT_AFFINE, window_bits=window_bits)
        ragged = fetch()
        assert (equal == ragged).all()
        for j in range(k):
            assert same(equal[j], be.msm(bases[j], scs[j])), j
        lens = [n, 0, 1]
        engine.msm_device_batch_items(curve, group, items(), out_form=OUT_AFFINE, window_bits=window_bits)
        ragged = fetch()
        assert (ragged[0] == equal[0]).all()
        assert same(ragged[1], be.zero) and same(ragged[2], be.msm(bases[2][:1], scs[2][:1]))
    finally:
        dev.free()


FOLD_CHILD = r'''
import ctypes, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import libff_amd
from oracle import port
port.build()
e = libff_amd.Engine(0)
curve, group, n = 1, 2, 300
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[vp(a) for a in arrs])
bases = [port.bases_seq(curve, group, n, first=500 * j) for j in range(2)]
scs = [port.scalars_sha512(curve, 3 + j, n) for j in range(2)]
wants = [port.multi_exp(curve, group, b, x, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True) for b, x in zip(bases, scs)]
assert libff_amd.plan(curve, group, n, window_bits=15)["num_buckets"] == 1 << 14
o = e._opts(window_bits=15, segment_len=2, out_form=libff_amd.OUT_AFFINE)
outs = np.zeros((3, libff_amd.sizes(curve, group)["g_bytes"] // 8), dtype=np.uint64)
rc = e.lib.amdmsm_multi_exp(e.h, curve, group, vp(bases[0]), ctypes.c_size_t(0), libff_amd.multi_exp_base_form_special,
                            vp(scs[0]), ctypes.c_size_t(n), vp(outs[0]), ctypes.byref(o))
assert rc == 0 and (outs[0] == wants[0]).all(), rc
rc = e.lib.amdmsm_multi_exp_batch(e.h, curve, group, 2, ptrs(bases), ctypes.c_size_t(0), libff_amd.multi_exp_base_form_special,
                                  ptrs(scs), ctypes.c_size_t(n), ptrs([outs[1], outs[2]]), ctypes.byref(o))
assert rc == 0 and (outs[1] == wants[0]).all() and (outs[2] == wants[1]).all(), rc
print("fold-child-ok")
'''


def test_fold_levels_of_the_segment_sums():
    """The segment kernels with more segments than one launch folds: AMDMSM_ROWCOL=0, bls12_377 G2, window_bits = 15 and
    segment_len = 2 give 2^14 / 2 = 8192 segments per window; k_reduce_segments folds 32 of them per wave, which leaves 256
    two-lane rows -- more than the 256 lanes of k_sum_block -- so one k_sum_butterfly level runs in front of it.  One
    MSM and a batch of two, each against the oracle."""
    code = FOLD_CHILD % (REPO, os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, AMDMSM_ROWCOL="0"))
    assert r.returncode == 0 and "fold-child-ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


CHILD = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import libff_amd
from libff_amd import BatchItem
from oracle import port
port.build()
e = libff_amd.Engine(0)
curve, group = 0, 1
lens = %r
shared = port.scalars_sha512(curve, 5, max(lens))
vecs = [port.bases_seq(curve, group, m, first=1000 * j) for j, m in enumerate(lens)]
idx = np.arange(lens[1], dtype=np.uint32)[::-1].copy()
items = [BatchItem(vecs[0]), BatchItem(vecs[1], index=idx), BatchItem(vecs[2], offset=7),
         BatchItem(vecs[3], scalars=port.scalars_sha512(curve, 6, lens[3]))]
sel = [shared[:lens[0]], shared[idx.astype(np.int64)], shared[7:7 + lens[2]], items[3].scalars]
wants = [port.multi_exp(curve, group, b, s, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True) for b, s in zip(vecs, sel)]
for rep in range(3):
    order = list(range(4)) if rep != 1 else [2, 0, 3, 1]
    got = e.multi_exp_batch_items(curve, group, [items[j] for j in order], shared, base_form=libff_amd.multi_exp_base_form_special)
    for pos, j in enumerate(order):
        assert (got[pos] == wants[j]).all(), (rep, j)
    assert (e.multi_exp(curve, group, vecs[3], sel[3], base_form=libff_amd.multi_exp_base_form_special) == wants[3]).all()
print("items-child-ok")
'''


@pytest.mark.parametrize("env,lens", [({"AMDMSM_BASE_CACHE_MB": "5"}, (1 << 14, 1 << 14, (1 << 14) - 7, 1 << 14)),
                                       ({"AMDMSM_MAX_RANGE_POINTS": "1000"}, (257, 3000, 64, 2500))],
                         ids=["base-cache-below-the-batch", "one-after-the-other-route"])
def test_child_process_settings(env, lens):
    """settings read once per process.  AMDMSM_BASE_CACHE_MB with a cap that holds two of the four vectors: resolved copies
    stay pinned for the call, the rest is uploaded.  AMDMSM_MAX_RANGE_POINTS below two of the lengths: the batch leaves
    the single pass and runs its MSMs one after the other, scalars gathered on the device."""
    code = CHILD % (REPO, os.path.join(REPO, "tests"), lens)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0 and "items-child-ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def _closed_form_k(plain, first, r):
    """sum_i plain_i * (first + i + 1) mod r for an (n, limbs) uint64 array of plain scalars"""
    n, fl = plain.shape
    lo32 = (plain & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    hi32 = (plain >> np.uint64(32)).astype(np.uint64)
    total = 0
    blk = 256   # 2^32 * 2^24 * 2^8 = 2^64: weights stay below 2^24 here
    for b0 in range(0, n, blk):
        w = np.arange(first + b0 + 1, first + min(b0 + blk, n) + 1, dtype=np.uint64)[:, None]
        lo = (lo32[b0:b0 + blk] * w).sum(axis=0, dtype=np.uint64)
        hi = (hi32[b0:b0 + blk] * w).sum(axis=0, dtype=np.uint64)
        for j in range(fl):
            total += (int(lo[j]) << (64 * j)) + (int(hi[j]) << (64 * j + 32))
    return total % r


@pytest.mark.parametrize("name,curve,group,log_m", [("alt_bn128_g1", 0, 1, 20), ("bls12_377_g1", 1, 1, 20), ("mnt4_g1", MNT4, G1, 16)])
def test_prover_shape_closed_form(engine, port, name, curve, group, log_m):
    """The four G1 MSMs of a Groth16 prover over device-generated bases (i + 1) G and one shared assignment of m + 1
    scalars: A the prefix (m + 1 terms), L the slice from l + 1 (l = 2^10), B a sorted index list of every second
    position, H an own vector of m - 1 terms.  Expected: (sum_i k_i (i + 1) mod r) G, test_multiexp.cpp:205-256."""
    m, l = 1 << log_m, 1 << 10
    bases = engine.gen_bases_seq(curve, group, m + 1)
    idx = np.arange(0, m + 1, 2, dtype=np.uint32)
    if name in MNT_MODELS:
        model = MNT_MODELS[name]
        rng = np.random.default_rng(log_m)
        mk = lambda cnt: np.concatenate([rng.integers(0, 1 << 63, size=(cnt, mm.WORDS - 1), dtype=np.uint64),
                                         rng.integers(0, 1 << 40, size=(cnt, 1), dtype=np.uint64)], axis=1)   # < 2^296 < r
        shared, own, plain_of, r = mk(m + 1), mk(m - 1), (lambda a: a), model.r
        point = lambda k: model.mul(k, model.one)
        canon = model.point
        kw = dict(scalars_plain=True)
    else:
        shared, own = port.scalars_sha512(curve, 0, m + 1), port.scalars_sha512(curve, 1, m - 1)
        plain_of = lambda a: port.fr_as_bigint(curve, a)
        r = to_int(golden()[f"{libff_amd.engine.CURVE_NAMES[curve]}_g1/fr_modulus"])
        one = port.group_consts(curve, group)[0]

        def point(k):
            kp = np.array([[(k >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(shared.shape[1])]], dtype=np.uint64)
            return tuple(port.group_op(curve, group, 4, port.scalar_mul(curve, group, one, port.fr_from_bigint(curve, kp)[0])))
        canon = tuple
        kw = {}
    items = [BatchItem(bases), BatchItem(bases[l + 1:], offset=l + 1), BatchItem(bases[:len(idx)], index=idx),
             BatchItem(bases[:m - 1], scalars=own)]
    got = engine.multi_exp_batch_items(curve, group, items, shared, base_form=multi_exp_base_form_special, **kw)
    ps = plain_of(shared)
    want = [point(_closed_form_k(ps, 0, r)), point(_closed_form_k(ps[l + 1:], l + 1, r)),
            point(_closed_form_k(ps[idx.astype(np.int64)], 0, r)), point(_closed_form_k(plain_of(own), 0, r))]
    for j in range(4):
        assert canon(got[j]) == want[j], j
