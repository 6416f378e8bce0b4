"""The streaming entries at their edges: the three reader-callback entries (Engine.multi_exp_stream) beside their _file
twins, all eleven groups -- chunk boundaries, one-record chunks, empty and one-element streams, zeros at the first and last
index of a chunk in both written forms, readers that deliver a few bytes at a time, streams that end early and the
context afterwards, a bad compressed record in a later chunk, records the reference wrote for the MNT groups, and a file
large enough for file_reader's threads.

No expectation comes from the device: results are compared with the oracle's multi_exp / multi_exp_precompute over the
same bases, or with the closed form of tests/mnt_model.py (tests/stream_cases.py, proven in test_stream_cases_cpu.py)."""
import os

import numpy as np
import pytest

import ffi_wire
import mnt_model as mm
import stream_cases as sc
from common import GROUPS, HERE, golden, to_int

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import multi_exp_base_form_special  # noqa: E402

BAD_ARG = -2
ALL = [g[0] for g in GROUPS] + sorted(ffi_wire.MNT_GROUPS)
A0 = [g[0] for g in GROUPS]   # the a = 0 groups: compressed records
N = max(sc.SIZES)
SENTINEL = 0xA5A5A5A5A5A5A5A5
_cases = {}


class Case:
    """193 bases with the zeros of stream_cases.zero_positions, their records, scalars, and the MSM of every prefix"""

    def __init__(self, port, name):
        self.name, self.port = name, port
        if name in ffi_wire.MNT_GROUPS:
            self.model, self.curve, self.group = ffi_wire.MNT_GROUPS[name]
            self.pts, self.ks, self.mult = sc.mnt_case(self.model, N)
            self.data, self.rec = sc.mnt_stream(self.model, self.pts)
            self.scalars = self.model.scalars_mont(self.ks)
            self.bases = self.model.records(self.pts)
        else:
            self.model = None
            _, self.curve, self.group = next(g for g in GROUPS if g[0] == name)
            self.bases = sc.oracle_bases(port, self.curve, self.group, N)
            self.data, self.rec = sc.oracle_stream(port, self.curve, self.group, self.bases)
            self.scalars = port.scalars_sha512(self.curve, 2024, N)
        assert len(self.data) == N * self.rec
        self._want = {}

    def check(self, got, n, what=""):
        """got: the OUT_AFFINE record of an MSM over the first n (base, scalar) pairs"""
        if self.model is not None:
            assert self.model.point(got) == sc.mnt_expect(self.model, self.ks, self.mult, n), (self.name, n, what)
            if n == 0:
                assert (got == self.model.records([mm.INF])[0]).all()
            return
        if n not in self._want:
            p = self.port
            self._want[n] = p.multi_exp(self.curve, self.group, self.bases[:n], self.scalars[:n], p.BDLO12_SIGNED, 1) if n \
                else p.group_consts(self.curve, self.group)[1]
        assert (got == self._want[n]).all(), (self.name, n, what)


def _case(port, name):
    if name not in _cases:
        _cases[name] = Case(port, name)
    return _cases[name]


def _both(engine, c, data, path, n, what, **kw):
    """the callback entry and its _file twin over the same records: bit-equal, and the callback took no byte too many"""
    rd = sc.Reader(data + sc.TRAILER)
    got = engine.multi_exp_stream(c.curve, c.group, rd, c.scalars[:n], **kw)
    want_bytes = n * len(data) // N
    assert rd.served == rd.requested == rd.asked == want_bytes, (what, n, rd.served, rd.requested, want_bytes)
    file_kw = dict(kw)
    if file_kw.pop("compressed", False):
        twin = engine.multi_exp_stream_compressed_file(c.curve, c.group, path, c.scalars[:n], **file_kw)
    elif "precompute_c" in file_kw:
        twin = engine.multi_exp_stream_with_precompute_file(c.curve, c.group, path, c.scalars[:n], file_kw.pop("precompute_c"), **file_kw)
    else:
        twin = engine.multi_exp_stream_file(c.curve, c.group, path, c.scalars[:n], **file_kw)
    assert (got == twin).all(), (what, n)
    return got


@pytest.mark.parametrize("name", ALL)
def test_uncompressed_sizes(engine, port, name, tmp_path):
    """n = 0, 1, k chunk - 1, k chunk, k chunk + 1 and a ragged tail at chunk_points = 64; five chunks of one record, so
    that each staging buffer is used again; chunk_points = 0.  Zeros stand at the last index of chunk 0 and the first of
    chunks 1 and 2, one of them written as (0, 0)."""
    c = _case(port, name)
    path = str(tmp_path / "bases.bin")
    with open(path, "wb") as f:
        f.write(c.data)
    for n in sc.SIZES:
        c.check(_both(engine, c, c.data, path, n, "chunk 64", chunk_points=sc.CHUNK), n, "chunk 64")
    c.check(_both(engine, c, c.data, path, 5, "chunk 1", chunk_points=1), 5, "chunk 1")
    c.check(_both(engine, c, c.data, path, N, "chunk 0", chunk_points=0), N, "chunk 0")


@pytest.mark.parametrize("name", A0)
def test_compressed_sizes(engine, port, name, tmp_path):
    c = _case(port, name)
    data = port.disk_write_compressed(c.curve, c.group, c.bases).tobytes()
    assert len(data) == N * c.rec // 2
    path = str(tmp_path / "bases_compressed.bin")
    with open(path, "wb") as f:
        f.write(data)
    for n in sc.SIZES:
        c.check(_both(engine, c, data, path, n, "compressed", chunk_points=sc.CHUNK, compressed=True), n, "compressed")
    c.check(_both(engine, c, data, path, 5, "compressed, chunk 1", chunk_points=1, compressed=True), 5)
    c.check(_both(engine, c, data, path, N, "compressed, chunk 0", chunk_points=0, compressed=True), N)


@pytest.mark.parametrize("name", ALL)
def test_precompute_sizes(engine, port, name, tmp_path):
    """multi_exp_stream_with_precompute at c = 9: the stream holds precompute_num_digits(curve, 9) multiples per base
    (the entry has no other digit count).  The table is the oracle's, or the model's doubling chains; for the MNT
    groups 34 digits of 9 bits leave the top digit spare bits, so no carry is lost and the result is the plain MSM."""
    c = _case(port, name)
    D = libff_amd.precompute_num_digits(c.curve, 9)
    if c.model is None:
        tab = port.precompute_table(c.curve, c.group, c.bases, 9)
        data = port.disk_write(c.curve, c.group, tab).tobytes()
    else:
        assert D * 9 > c.model.r.bit_length() + 1
        data = c.model.disk_write(sc.mnt_precompute_points(c.model, c.pts, 9, D))
    assert len(data) == N * D * c.rec
    path = str(tmp_path / "table.bin")
    with open(path, "wb") as f:
        f.write(data)
    for n in (1, 65, N):
        got = _both(engine, c, data, path, n, "precompute", chunk_points=sc.CHUNK, precompute_c=9)
        if c.model is None:
            want = port.multi_exp_precompute(c.curve, c.group, tab[:n * D], c.scalars[:n], 9)
            assert (got == want).all(), (name, n)
        else:
            c.check(got, n, "precompute")


@pytest.mark.parametrize("name", sorted(ffi_wire.MNT_GROUPS))
def test_mnt_records_of_the_reference(engine, name, tmp_path):
    """the 10-word records of the MNT groups (the 8-byte load path of k_disk_decode) as the reference's writer left them"""
    model, curve, group = ffi_wire.MNT_GROUPS[name]
    f = dict(np.load(os.path.join(HERE, "golden", "mnt_disk.npz")))
    pts = [model.point(row) for row in f[f"{name}/elems"]]
    data = f[f"{name}/disk_bytes"].tobytes()
    ks = [0, 1, model.r - 1, 5, 1 << 297, 123456789 ** 4, model.r // 3][:len(pts)]
    want = model.msm(pts, ks)
    path = str(tmp_path / "mnt.bin")
    with open(path, "wb") as fh:
        fh.write(data)
    for chunk in (0, 3, 1):
        got = engine.multi_exp_stream(curve, group, sc.Reader(data), model.scalars_mont(ks), chunk_points=chunk)
        assert model.point(got) == want, chunk
        twin = engine.multi_exp_stream_file(curve, group, path, model.scalars_mont(ks), chunk_points=chunk)
        assert (twin == got).all(), chunk


PIECE_GROUPS = ["alt_bn128_g1", "bls12_377_g2"]   # a prime-field group and an Fq2 group


@pytest.mark.parametrize("policy", sc.POLICIES + [("fixed", 1)], ids=str)
@pytest.mark.parametrize("name", PIECE_GROUPS)
def test_piece_policies(engine, port, name, policy):
    """a reader that delivers whole requests, 7 bytes a time (never aligned to a word or a record), random pieces, one
    byte a time: the same result, and not a byte taken beyond the n records although the stream holds more"""
    c = _case(port, name)
    n = 65 if policy == ("fixed", 1) else N
    rd = sc.Reader(c.data + sc.TRAILER, policy)
    got = engine.multi_exp_stream(c.curve, c.group, rd, c.scalars[:n], chunk_points=sc.CHUNK)
    c.check(got, n, policy)
    assert rd.served == n * c.rec and rd.requested == n * c.rec, (rd.served, rd.requested, n * c.rec)
    if policy == "whole":
        assert rd.asked == n * c.rec and rd.calls == -(-n // sc.CHUNK)


@pytest.mark.parametrize("where", ["inside chunk 0", "inside chunk 2", "at the end of chunk 1"])
@pytest.mark.parametrize("name", PIECE_GROUPS)
def test_end_of_stream(engine, port, name, where, tmp_path):
    """the stream ends early: BAD_ARG, "ended early", the output untouched -- and the context, whose pipeline depth and
    slot rotation the call changes, serves a plain multi_exp and a full stream afterwards"""
    c = _case(port, name)
    end = {"inside chunk 0": 10 * c.rec + 5, "inside chunk 2": (2 * sc.CHUNK + 10) * c.rec + 5,
           "at the end of chunk 1": 2 * sc.CHUNK * c.rec}[where]
    path = str(tmp_path / "short.bin")
    with open(path, "wb") as f:
        f.write(c.data[:end])
    for policy in ("whole", ("fixed", 7)):
        out = np.full(c.bases.shape[1], SENTINEL, dtype=np.uint64)
        rd = sc.Reader(c.data, policy, end_at=end)
        with pytest.raises(libff_amd.AmdMsmError) as ei:
            engine.multi_exp_stream(c.curve, c.group, rd, c.scalars, chunk_points=sc.CHUNK, out=out)
        assert ei.value.code == BAD_ARG and "ended early" in str(ei.value), str(ei.value)
        assert (out == SENTINEL).all() and rd.served == end
    with pytest.raises(libff_amd.AmdMsmError) as ei:
        engine.multi_exp_stream_file(c.curve, c.group, path, c.scalars, chunk_points=sc.CHUNK)
    assert ei.value.code == BAD_ARG and "ended early" in str(ei.value), str(ei.value)
    got = engine.multi_exp(c.curve, c.group, c.bases, c.scalars, base_form=multi_exp_base_form_special)
    c.check(got, N, "multi_exp after the failure")
    got = engine.multi_exp_stream(c.curve, c.group, sc.Reader(c.data), c.scalars, chunk_points=sc.CHUNK)
    c.check(got, N, "stream after the failure")


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_381_g2"])
def test_bad_compressed_record_in_a_later_chunk(engine, port, name, tmp_path):
    """an X with no point above it in chunk 2 of 4 fails the call; the same call with the good bytes then succeeds"""
    _, curve, group = next(g for g in GROUPS if g[0] == name)
    n, cb = 4 * sc.CHUNK, port.sizes(curve, group)["coord_bytes"]
    bases = port.bases_seq(curve, group, n, first=9)
    scal = port.scalars_sha512(curve, 321, n)
    rec = port.disk_write_compressed(curve, group, bases)
    idx = 2 * sc.CHUNK + 7
    bad = None
    for delta in range(1, 60):
        r2 = rec.copy()
        r2[idx * cb + cb - 1] = (int(r2[idx * cb + cb - 1]) + delta) & 0xFF
        if port.disk_read_compressed(curve, group, r2[idx * cb:(idx + 1) * cb], 1)[1] == 1:
            bad = r2
            break
    assert bad is not None
    want = port.multi_exp(curve, group, bases, scal, port.BDLO12_SIGNED, 1)
    path = str(tmp_path / "c.bin")
    for data, ok in ((bad.tobytes(), False), (rec.tobytes(), True)):
        with open(path, "wb") as f:
            f.write(data)
        calls = [lambda out: engine.multi_exp_stream(curve, group, sc.Reader(data), scal, chunk_points=sc.CHUNK, compressed=True, out=out),
                 lambda out: engine.multi_exp_stream_compressed_file(curve, group, path, scal, chunk_points=sc.CHUNK)]
        for call in calls:
            out = np.full(bases.shape[1], SENTINEL, dtype=np.uint64)
            if ok:
                assert (call(out) == want).all()
            else:
                with pytest.raises(libff_amd.AmdMsmError) as ei:
                    call(out)
                assert ei.value.code == BAD_ARG and "not on the curve" in str(ei.value), str(ei.value)
                assert (out == SENTINEL).all()


def test_threaded_file_reader(engine, port, tmp_path):
    """A chunk of 12 MiB -- two 8 MiB slices, read by two threads of file_reader with pread at their own offsets: 48
    copies of a block of 4096 alt_bn128 G1 records, every position with a scalar of its own.  The copies of the second
    slice hold the negated block (a slice read from the wrong offset of a purely periodic file would go unnoticed), so
    the expectation is the oracle's MSM over the block with the scalars of each position summed, with that sign, mod r.
    A file cut inside the second slice, or one record short, fails."""
    curve, group, block, copies, first_neg = 0, 1, 4096, 48, 32
    r = to_int(golden()["alt_bn128_g1/fr_modulus"])
    bases = port.bases_seq(curve, group, block, first=100)
    bases[17] = port.group_consts(curve, group)[1]
    neg = np.stack([port.group_op(curve, group, 3, b) for b in bases])
    pos_bytes, neg_bytes = port.disk_write(curve, group, bases).tobytes(), port.disk_write(curve, group, neg).tobytes()
    assert len(pos_bytes) == block * 64 and first_neg * len(pos_bytes) == 8 << 20
    ks, summed = sc.tiled_scalars(r, block, copies, seed=48, first_neg=first_neg)
    scal = sc.plain_records([k for row in ks for k in row], 4)
    want = port.multi_exp(curve, group, bases, port.fr_from_bigint(curve, sc.plain_records(summed, 4)), port.BDLO12_SIGNED, 1)
    path = str(tmp_path / "tiled.bin")
    with open(path, "wb") as f:
        for c in range(copies):
            f.write(pos_bytes if c < first_neg else neg_bytes)
    assert os.path.getsize(path) == 12 << 20
    got = engine.multi_exp_stream_file(curve, group, path, scal, chunk_points=0, scalars_plain=True)
    assert (got == want).all()
    for size in ((8 << 20) + 1000, (12 << 20) - 64):
        os.truncate(path, size)
        with pytest.raises(libff_amd.AmdMsmError) as ei:
            engine.multi_exp_stream_file(curve, group, path, scal, chunk_points=0, scalars_plain=True)
        assert ei.value.code == BAD_ARG and "ended early" in str(ei.value), (size, str(ei.value))
