"""The reader, the inputs and the expectations of tests/test_gpu_stream_readers.py (tests/stream_cases.py) proven
without a device, and the MNT record writer of tests/mnt_model.py against records the reference wrote
(tests/golden/mnt_disk.npz, tests/golden/make_mnt_disk_golden.py)."""
import os

import numpy as np
import pytest

import ffi_wire
import mnt_model as mm
import stream_cases as sc
from common import HERE, golden, to_int


def _mnt_disk():
    return dict(np.load(os.path.join(HERE, "golden", "mnt_disk.npz")))


@pytest.mark.parametrize("name", sorted(ffi_wire.MNT_GROUPS))
def test_mnt_writer_reproduces_the_references_records(name):
    model = ffi_wire.MNT_GROUPS[name][0]
    f = _mnt_disk()
    elems, want = f[f"{name}/elems"], f[f"{name}/disk_bytes"].tobytes()
    pts = [model.point(row) for row in elems]
    assert len(pts) <= 8 and mm.INF in pts and any(p is not mm.INF for p in pts)
    assert any(to_int(row[2 * model.cw:]) not in (0, to_int(model.records([model.one])[0][2 * model.cw:])) for row in elems), \
        "no element with Z != 1: the writer's normalisation is not exercised"
    assert model.disk_write(pts) == want
    assert len(want) == len(pts) * 2 * 8 * mm.WORDS * model.deg


def test_tiled_file_expectation(port):
    """the MSM over 3 copies of a block of 64 records, a scalar of its own per position, is the MSM over the block with
    the scalars of each position summed mod r"""
    curve, group, block, copies = 0, 1, 64, 3
    r = to_int(golden()["alt_bn128_g1/fr_modulus"])
    limbs = port.sizes(curve, group)["fr_bytes"] // 8
    bases = port.bases_seq(curve, group, block, first=30)
    ks, summed = sc.tiled_scalars(r, block, copies, seed=4)
    flat = [k for row in ks for k in row]
    tiled = np.concatenate([bases] * copies)
    want = port.multi_exp(curve, group, tiled, port.fr_from_bigint(curve, sc.plain_records(flat, limbs)), port.BDLO12_SIGNED, 1)
    got = port.multi_exp(curve, group, bases, port.fr_from_bigint(curve, sc.plain_records(summed, limbs)), port.BDLO12_SIGNED, 1)
    assert (got == want).all()
    # the last copy negated, as the file of the threaded reader has its second slice
    ks, summed = sc.tiled_scalars(r, block, copies, seed=5, first_neg=2)
    flat = [k for row in ks for k in row]
    neg = np.stack([port.group_op(curve, group, 3, x) for x in bases])
    tiled = np.concatenate([bases, bases, neg])
    want = port.multi_exp(curve, group, tiled, port.fr_from_bigint(curve, sc.plain_records(flat, limbs)), port.BDLO12_SIGNED, 1)
    got = port.multi_exp(curve, group, bases, port.fr_from_bigint(curve, sc.plain_records(summed, limbs)), port.BDLO12_SIGNED, 1)
    assert (got == want).all()
    assert (sc.plain_records([5, 1 << 200], limbs) == np.array([[5, 0, 0, 0], [0, 0, 0, 1 << 8]], dtype=np.uint64)).all()


@pytest.mark.parametrize("policy", sc.POLICIES + [("fixed", 1)], ids=str)
def test_reader_policies_deliver_the_source_bytes(policy):
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, size=193 * 64, dtype=np.uint8).tobytes()
    rd = sc.Reader(data + sc.TRAILER, policy)
    got = b"".join(rd.drain(min(64 * 64, len(data) - off)) for off in range(0, len(data), 64 * 64))
    assert got == data
    assert rd.served == rd.requested == len(data), "the drain loop never asks beyond what it still needs"
    if policy == "whole":
        assert rd.asked == len(data) and rd.calls == 4
    else:
        assert rd.asked > len(data) and rd.calls > 4
    if policy == ("fixed", 7):
        assert rd.calls == sum(-(-min(4096, len(data) - off) // 7) for off in range(0, len(data), 4096))
    # a consumer that asks for more than it needs is seen to
    greedy = sc.Reader(data + sc.TRAILER, policy)
    greedy.drain(100, ask=lambda left: left + 1)
    assert greedy.requested > 100


@pytest.mark.parametrize("policy", sc.POLICIES, ids=str)
def test_reader_ends_early(policy):
    data = bytes(range(256)) * 40
    end = 10 * 64 + 5
    rd = sc.Reader(data, policy, end_at=end)
    assert rd.drain(64 * 64) == data[:end]
    assert rd(100) == b"" and rd.served == end


def test_stream_inputs(port):
    assert sc.zero_positions(193) == [63, 64, 128] and sc.zero_positions(64) == [63] and sc.zero_positions(1) == []
    assert sc.zero_positions(5, chunk=1) == [0, 1, 2]
    curve, group = 0, 2
    bases = sc.oracle_bases(port, curve, group, 65)
    data, rec = sc.oracle_stream(port, curve, group, bases)
    assert len(data) == 65 * rec
    plain = port.disk_write(curve, group, bases).tobytes()
    assert data[:64 * rec] == plain[:64 * rec] and data[64 * rec:] == bytes(rec) != plain[64 * rec:]
    # the MNT case: bases, records and the closed form of their MSM
    model = mm.MNT4
    pts, ks, mult = sc.mnt_case(model, 66)
    assert pts[0] == model.mul(9, model.one) and pts[63] is mm.INF and pts[64] is mm.INF and pts[65] == model.mul(74, model.one)
    assert sc.mnt_expect(model, ks, mult, 66) == model.msm(pts, ks)
    assert sc.mnt_expect(model, ks, mult, 0) is mm.INF
    tab = sc.mnt_precompute_points(model, pts[:2], 9, 3)
    assert tab == [pts[0], model.mul(9 << 9, model.one), model.mul(9 << 18, model.one),
                   pts[1], model.mul(10 << 9, model.one), model.mul(10 << 18, model.one)]
