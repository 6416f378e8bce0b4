"""The on-disk encoders (Engine.disk_encode / disk_encode_device) and the stream and file writers (write_points_stream /
write_points_file), all eleven groups: the bytes of the reference's writer (tests/golden), the oracle's writer and the MNT
model's over bases with both parities of Y and zeros at the first index, the last and the chunk boundaries; sizes around
a workgroup; sentinels behind the records; round trips through the decoder; chunked writes, offsets and trailers, writers
that stop early, bad paths; the written files through the stream readers; the precompute file.

No expectation comes from the device: bytes are compared with committed reference bytes, oracle/port.py or
tests/mnt_model.py, MSM results with the oracle's multi_exp or the model's closed form (tests/stream_cases.py)."""
import os

import numpy as np
import pytest

import ffi_wire
import mnt_model as mm
import stream_cases as sc
from common import GROUPS, HERE, golden, literal

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import multi_exp_base_form_normal, multi_exp_base_form_special  # noqa: E402

BAD_ARG, UNSUPPORTED = -2, -3
ALL = [g[0] for g in GROUPS] + sorted(ffi_wire.MNT_GROUPS)
A0 = [g[0] for g in GROUPS]   # the a = 0 groups: compressed records
N = 257
ENCODE_SIZES = (0, 1, 255, 256, 257)   # one lane per record, 256 lanes per workgroup
SENTINEL = 0xA5
_cases = {}


class Case:
    """257 bases (k + 9) G with the zeros of stream_cases.zero_positions (chunk 64: indices 63, 64, 128) and one negated
    point, so that both parities of Y occur; their records by the oracle or the model; scalars and the MSM of a prefix"""

    def __init__(self, port, name):
        self.name, self.port = name, port
        if name in ffi_wire.MNT_GROUPS:
            self.model, self.curve, self.group = ffi_wire.MNT_GROUPS[name]
            self.pts, self.ks, self.mult = sc.mnt_case(self.model, N)
            self.pts[1], self.mult[1] = self.model.neg(self.pts[1]), -self.mult[1]   # a negated point among them
            self.bases = self.model.records(self.pts)
            self.scalars = self.model.scalars_mont(self.ks)
            self.zero = self.model.records([mm.INF])[0]
        else:
            self.model = None
            _, self.curve, self.group = next(g for g in GROUPS if g[0] == name)
            self.bases = sc.oracle_bases(port, self.curve, self.group, N)
            y0 = self.bases.shape[1] // 3   # word 0 of Y (of Y.c0), whose low bit the compressed record keeps
            if (int(self.bases[1][y0]) ^ int(self.bases[2][y0])) & 1 == 0:
                self.bases[1] = port.group_op(self.curve, self.group, 3, self.bases[1])   # -P: the other parity, q being odd
            assert (int(self.bases[1][y0]) ^ int(self.bases[2][y0])) & 1 == 1, "both parities of Y"
            self.scalars = port.scalars_sha512(self.curve, 2024, N)
            self.zero = port.group_consts(self.curve, self.group)[1]
        s = libff_amd.sizes(self.curve, self.group)
        self.rec, self.g_bytes, self.aff_bytes = s["affine_bytes"], s["g_bytes"], s["affine_bytes"]
        self._want = {}

    def with_zero_ends(self, n):
        """the first n bases, the first and the last of them zero"""
        b = self.bases[:n].copy()
        if n:
            b[0] = self.zero
            b[n - 1] = self.zero
        return b

    def records(self, bases, compressed=False):
        """the on-disk records of `bases`, by the oracle's writer or the model's"""
        if bases.shape[0] == 0:
            return b""
        if self.model is not None:
            assert not compressed
            return self.model.disk_write([self.model.point(row) for row in bases])
        w = self.port.disk_write_compressed if compressed else self.port.disk_write
        return w(self.curve, self.group, bases).tobytes()

    def special(self, bases):
        """every record in special form, what disk_decode returns"""
        if self.model is not None:
            return self.model.records([self.model.point(row) for row in bases])
        return np.stack([self.port.group_op(self.curve, self.group, 4, row) for row in bases])

    def check_msm(self, got, n, what=""):
        """got: the OUT_AFFINE record of the MSM over the first n (base, scalar) pairs"""
        if self.model is not None:
            want = self.model.mul(sum(k * m for k, m in zip(self.ks[:n], self.mult[:n])) % self.model.r, self.model.one)
            assert self.model.point(got) == want, (self.name, n, what)
            return
        if n not in self._want:
            p = self.port
            self._want[n] = p.multi_exp(self.curve, self.group, self.bases[:n], self.scalars[:n], p.BDLO12_SIGNED, 1) if n \
                else self.zero
        assert (got == self._want[n]).all(), (self.name, n, what)


def _case(port, name):
    if name not in _cases:
        _cases[name] = Case(port, name)
    return _cases[name]


class Resident:
    """libff records uploaded and imported: compact affine records in HBM for the length of a ``with`` block"""

    def __init__(self, engine, curve, group, xyz, base_form=multi_exp_base_form_normal, extra=()):
        self.e, self.n = engine, xyz.shape[0]
        s = libff_amd.sizes(curve, group)
        self.ptrs = [engine.malloc(max(16, xyz.nbytes)), engine.malloc(max(16, self.n * s["affine_bytes"]))]
        self.ptrs += [engine.malloc(max(16, b)) for b in extra]
        if self.n:
            engine.h2d(self.ptrs[0], xyz)
            engine.import_bases_device(curve, group, self.ptrs[0], s["g_bytes"], base_form, self.n, self.ptrs[1])
        engine.synchronize()
        self.aff = self.ptrs[1]
        self.extra = self.ptrs[2:]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.synchronize()
        for p in self.ptrs:
            self.e.free(p)


class Writer:
    """``writer.write(bytes)``: keeps every call; from call `short_at` on it takes half of what it is given"""

    def __init__(self, short_at=None):
        self.calls, self.short_at = [], short_at

    def write(self, data):
        assert isinstance(data, bytes)
        if self.short_at is not None and len(self.calls) >= self.short_at:
            self.calls.append(data[:len(data) // 2])
            return len(data) // 2
        self.calls.append(data)
        return len(data)

    def data(self):
        return b"".join(self.calls)


# ---- the encoders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,curve,group", GROUPS)
def test_bytes_of_the_reference_writer(engine, name, curve, group):
    """the six elements the reference wrote (affine, zero, non-normalised) and its five curve points outside the subgroup"""
    g = golden()
    elems = g[f"{name}/disk_elems"]
    assert (engine.disk_encode(curve, group, elems) == g[f"{name}/disk_bytes"]).all()
    assert (engine.disk_encode(curve, group, elems, compressed=True) == g[f"{name}/disk_bytes_compressed"]).all()
    cp = g[f"{name}/curve_points"]
    assert (engine.disk_encode(curve, group, cp, compressed=True) == g[f"{name}/curve_points_compressed"]).all()
    # bytes -> points -> bytes
    for key, compressed in (("disk_bytes", False), ("disk_bytes_compressed", True), ("curve_points_compressed", True)):
        n = g[f"{name}/{key}"].size // (libff_amd.sizes(curve, group)["affine_bytes"] // (2 if compressed else 1))
        pts, status = engine.disk_decode(curve, group, g[f"{name}/{key}"], n, compressed=compressed)
        assert status == 0
        again = engine.disk_encode(curve, group, pts, compressed=compressed, base_form=multi_exp_base_form_special)
        assert (again == g[f"{name}/{key}"]).all(), key


@pytest.mark.parametrize("name", sorted(ffi_wire.MNT_GROUPS))
def test_mnt_bytes_of_the_reference_writer(engine, name):
    """the 10-word fields: 8-byte stores, 80- and 160-byte records"""
    model, curve, group = ffi_wire.MNT_GROUPS[name]
    f = dict(np.load(os.path.join(HERE, "golden", "mnt_disk.npz")))
    elems, want = f[f"{name}/elems"], f[f"{name}/disk_bytes"]
    assert (engine.disk_encode(curve, group, elems) == want).all()
    pts, status = engine.disk_decode(curve, group, want, elems.shape[0], compressed=False)
    assert status == 0
    assert (engine.disk_encode(curve, group, pts, base_form=multi_exp_base_form_special) == want).all()
    with pytest.raises(libff_amd.AmdMsmError) as ei:
        engine.disk_encode(curve, group, elems, compressed=True)
    assert ei.value.code == UNSUPPORTED and "compressed records: a != 0 curve" in str(ei.value)


@pytest.mark.parametrize("name", ALL)
def test_against_the_oracle_writer(engine, port, name):
    """n = 0, 1, 255, 256, 257 with zeros at index 0 and n - 1 besides those at 63, 64 and 128, both parities of Y;
    and the way back through the decoder"""
    c = _case(port, name)
    forms = (False, True) if name in A0 else (False,)
    for n in ENCODE_SIZES:
        for bases in (c.bases[:n], c.with_zero_ends(n)):
            for compressed in forms:
                got = engine.disk_encode(c.curve, c.group, bases, compressed=compressed, base_form=multi_exp_base_form_special)
                assert got.tobytes() == c.records(bases, compressed), (name, n, compressed)
    bases = c.with_zero_ends(N)
    want = c.special(bases)
    for compressed in forms:
        data = engine.disk_encode(c.curve, c.group, bases, compressed=compressed, base_form=multi_exp_base_form_special)
        back, status = engine.disk_decode(c.curve, c.group, data, N, compressed=compressed)
        assert status == 0 and (back == want).all(), (name, compressed)


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bw6_761_g2", "mnt4_g2"])
def test_sentinels_and_the_source(engine, port, name):
    """nothing is written behind the n records, nothing in front of a vector that starts inside an allocation, and the
    source keeps its bytes"""
    c = _case(port, name)
    for compressed in ((False, True) if name in A0 else (False,)):
        rec = c.rec // 2 if compressed else c.rec
        for n in (1, 255, 257):
            pad = 4 * rec
            with Resident(engine, c.curve, c.group, c.bases[:n], multi_exp_base_form_special, extra=(n * rec + 2 * pad,)) as r:
                buf = np.full(n * rec + 2 * pad, SENTINEL, dtype=np.uint8)
                src_before = np.zeros(n * c.aff_bytes, dtype=np.uint8)
                engine.h2d(r.extra[0], buf)
                engine.d2h(src_before, r.aff)
                engine.disk_encode_device(c.curve, c.group, r.aff.value, n, r.extra[0].value + pad, compressed=compressed)
                engine.synchronize()
                engine.d2h(buf, r.extra[0])
                src_after = np.zeros_like(src_before)
                engine.d2h(src_after, r.aff)
            assert (buf[:pad] == SENTINEL).all() and (buf[pad + n * rec:] == SENTINEL).all(), (name, n, compressed)
            assert buf[pad:pad + n * rec].tobytes() == c.records(c.bases[:n], compressed), (name, n, compressed)
            assert (src_before == src_after).all()


def test_refusals_of_the_device_encoder(engine, port):
    c = _case(port, "alt_bn128_g1")
    with Resident(engine, c.curve, c.group, c.bases[:8], multi_exp_base_form_special, extra=(1024,)) as r:
        aff, rec = r.aff.value, r.extra[0].value
        buf = np.full(1024, SENTINEL, dtype=np.uint8)
        engine.h2d(r.extra[0], buf)
        for args, text in (((None, 8, rec), "null pointer"), ((aff, 8, None), "null pointer"),
                           ((aff + 4, 4, rec), "d_points_affine: not aligned to 16 bytes"),
                           ((aff, 8, rec + 8), "d_records: not aligned to 16 bytes"),
                           ((aff, 8, aff + 64), "d_records overlaps d_src_affine"), ((aff, 8, aff), "d_records overlaps d_src_affine")):
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                engine.disk_encode_device(c.curve, c.group, args[0], args[1], args[2])
            assert ei.value.code == BAD_ARG and text in str(ei.value), (args, str(ei.value))
        engine.disk_encode_device(c.curve, c.group, None, 0, None)   # n = 0 succeeds
        engine.synchronize()
        engine.d2h(buf, r.extra[0])
        assert (buf == SENTINEL).all()
    with pytest.raises(libff_amd.AmdMsmError) as ei:
        engine.disk_encode_device(5, 2, None, 0, None)
    assert ei.value.code == UNSUPPORTED


# ---- the stream and file writers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_chunked_writes(engine, port, name, tmp_path):
    """chunk_points = 64 at n = 0, 1, 63, 64, 65, 128, 193, five chunks of one record, chunk_points = 0: the bytes of the
    oracle's writer, one call per chunk and in order; the file twin behind a 24-byte header and in front of a trailer"""
    c = _case(port, name)
    forms = (False, True) if name in A0 else (False,)
    with Resident(engine, c.curve, c.group, c.bases, multi_exp_base_form_special) as r:
        for compressed in forms:
            rec = c.rec // 2 if compressed else c.rec
            whole = c.records(c.bases, compressed)
            for n, chunk in [(n, sc.CHUNK) for n in sc.SIZES] + [(5, 1), (max(sc.SIZES), 0)]:
                w = Writer()
                engine.write_points_stream(c.curve, c.group, r.aff, n, w, compressed=compressed, chunk_points=chunk)
                size = min(chunk or 1 << 20, n)
                assert [len(x) for x in w.calls] == [min(size, n - lo) * rec for lo in range(0, n, size or 1)], (name, n, chunk)
                assert w.data() == whole[:n * rec], (name, n, chunk, compressed)
                path = str(tmp_path / f"{name}_{n}_{chunk}_{int(compressed)}.bin")
                header = bytes(range(24))
                with open(path, "wb") as f:
                    f.write(header + b"\x11" * (n * rec) + sc.TRAILER)
                engine.write_points_file(c.curve, c.group, r.aff, n, path, offset_bytes=24, compressed=compressed, chunk_points=chunk)
                with open(path, "rb") as f:
                    assert f.read() == header + whole[:n * rec] + sc.TRAILER, (name, n, chunk, compressed)
        # a file that does not exist yet is created; the gap in front of the offset reads as zeros
        path = str(tmp_path / "fresh.bin")
        engine.write_points_file(c.curve, c.group, r.aff, 65, path, offset_bytes=24, chunk_points=sc.CHUNK)
        with open(path, "rb") as f:
            assert f.read() == bytes(24) + c.records(c.bases[:65])


@pytest.mark.parametrize("name", ["alt_bn128_g1", "bls12_377_g2", "mnt6_g1"])
def test_a_writer_that_stops_early(engine, port, name, tmp_path):
    """half of the second chunk taken: BAD_ARG, "ended early", two calls seen -- and the context writes again"""
    c = _case(port, name)
    with Resident(engine, c.curve, c.group, c.bases, multi_exp_base_form_special) as r:
        for short_at in (1, 0, 3):
            w = Writer(short_at=short_at)
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                engine.write_points_stream(c.curve, c.group, r.aff, 193, w, chunk_points=sc.CHUNK)
            assert ei.value.code == BAD_ARG and "ended early" in str(ei.value), str(ei.value)
            assert len(w.calls) == short_at + 1
            assert b"".join(w.calls[:short_at]) == c.records(c.bases[:short_at * sc.CHUNK])
            w = Writer()
            engine.write_points_stream(c.curve, c.group, r.aff, 193, w, chunk_points=sc.CHUNK)
            assert w.data() == c.records(c.bases[:193])

        class Boom:
            def write(self, data):
                raise KeyError("boom")

        with pytest.raises(KeyError):
            engine.write_points_stream(c.curve, c.group, r.aff, 5, Boom(), chunk_points=1)
        for path in (str(tmp_path / "no_such_dir" / "x.bin"), str(tmp_path)):
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                engine.write_points_file(c.curve, c.group, r.aff, 5, path)
            assert ei.value.code == BAD_ARG and "cannot open" in str(ei.value), str(ei.value)
        never = str(tmp_path / "never.bin")   # a refused call creates no file
        for d_points, text in ((None, "null pointer"), (r.aff.value + 4, "d_points_affine: not aligned")):
            with pytest.raises(libff_amd.AmdMsmError) as ei:
                engine.write_points_file(c.curve, c.group, d_points, 5, never)
            assert ei.value.code == BAD_ARG and text in str(ei.value) and not os.path.exists(never), str(ei.value)
        got = np.zeros(c.g_bytes // 8, dtype=np.uint64)
        with Resident(engine, c.curve, c.group, c.bases[:0], extra=(c.scalars.nbytes, c.g_bytes)) as t:
            engine.h2d(t.extra[0], c.scalars)
            engine.msm_device(c.curve, c.group, r.aff, t.extra[0], 193, t.extra[1], out_form=libff_amd.OUT_AFFINE)
            engine.synchronize()
            engine.d2h(got, t.extra[1])
        c.check_msm(got, 193, "msm_device after the failures")


@pytest.mark.parametrize("name", ALL)
def test_written_files_through_the_readers(engine, port, name, tmp_path):
    """write_points_file, then multi_exp_stream_file (and the compressed pair for a = 0) over the file: the MSM of
    msm_device over the same resident points, which is the oracle's / the model's"""
    c = _case(port, name)
    n = 193
    with Resident(engine, c.curve, c.group, c.bases, multi_exp_base_form_special, extra=(c.scalars.nbytes, c.g_bytes)) as r:
        engine.h2d(r.extra[0], c.scalars)
        resident = np.zeros(c.g_bytes // 8, dtype=np.uint64)
        engine.msm_device(c.curve, c.group, r.aff, r.extra[0], n, r.extra[1], out_form=libff_amd.OUT_AFFINE)
        engine.synchronize()
        engine.d2h(resident, r.extra[1])
        c.check_msm(resident, n, "msm_device")
        path = str(tmp_path / "points.bin")
        engine.write_points_file(c.curve, c.group, r.aff, n, path, chunk_points=sc.CHUNK)
        assert os.path.getsize(path) == n * c.rec
        for chunk in (sc.CHUNK, 0):
            got = engine.multi_exp_stream_file(c.curve, c.group, path, c.scalars[:n], chunk_points=chunk)
            assert (got == resident).all(), (name, chunk)
        if name in A0:
            path = str(tmp_path / "points_compressed.bin")
            engine.write_points_file(c.curve, c.group, r.aff, n, path, compressed=True, chunk_points=sc.CHUNK)
            assert os.path.getsize(path) == n * c.rec // 2
            got = engine.multi_exp_stream_compressed_file(c.curve, c.group, path, c.scalars[:n], chunk_points=50)
            assert (got == resident).all(), name


@pytest.mark.parametrize("name,curve,group", GROUPS)
def test_the_precompute_file(engine, port, name, curve, group, tmp_path):
    """amdmsm_precompute_bases_device -> write_points_file: the file profile_multiexp.cpp's create_precompute_file_for_config
    would write -- the oracle's table through the oracle's writer, byte for byte -- and through
    multi_exp_stream_with_precompute_file the results the reference recorded"""
    g, lit = golden(), literal()["groups"][name]
    nb = 24
    bases = port.bases_r32(curve, group, nb)
    sc70 = port.scalars_sha512(curve, 70, nb)
    s = libff_amd.sizes(curve, group)
    for c in lit["precompute_c"]:
        D = libff_amd.precompute_num_digits(curve, c)
        want = port.disk_write(curve, group, port.precompute_table(curve, group, bases, c)).tobytes()
        path = str(tmp_path / f"table_{c}.bin")
        with Resident(engine, curve, group, bases, multi_exp_base_form_special, extra=(nb * D * s["affine_bytes"],)) as r:
            engine.precompute_bases_device(curve, group, r.aff, nb, c, D, r.extra[0])
            engine.write_points_file(curve, group, r.extra[0], nb * D, path, chunk_points=100)
        with open(path, "rb") as f:
            assert f.read() == want, c
        for chunk in (0, 7):
            got = engine.multi_exp_stream_with_precompute_file(curve, group, path, sc70, c, chunk_points=chunk)
            assert (got == g[f"{name}/pre_c{c}_msm"]).all(), (c, chunk)
