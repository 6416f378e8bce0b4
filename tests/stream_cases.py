"""The reader, the inputs and the expectations of the streaming tests (tests/test_gpu_stream_readers.py), device-free:
tests/test_stream_cases_cpu.py proves them against the oracle."""
import random

import numpy as np

import mnt_model as mm

CHUNK = 64
SIZES = (0, 1, 63, 64, 65, 128, 193)   # with chunk_points = 64: n = k chunk - 1, k chunk, k chunk + 1, a ragged tail
TRAILER = b"\xee" * 1000               # what follows the records in a stream that holds more


class Reader:
    """``reader(nbytes) -> bytes`` of Engine.multi_exp_stream over a bytes object.
    policy: "whole" -- every request in full; ("fixed", k) -- at most k bytes a time; ("random", seed) -- seeded pieces
    of 1 to 4096 bytes.  end_at: the stream ends at that offset, whatever ``data`` holds beyond.
    It records: calls; asked, the bytes of all requests added up (a request the reader serves in part is followed by
    one for the rest, so this counts a byte once only with "whole"); requested, the furthest offset any request reached
    -- what a consumer of a pipe would have taken out of it; served, the bytes delivered."""

    def __init__(self, data, policy="whole", end_at=None):
        self.data, self.policy = bytes(data), policy
        self.end = len(self.data) if end_at is None else end_at
        assert 0 <= self.end <= len(self.data)
        self.rng = random.Random(policy[1]) if policy != "whole" and policy[0] == "random" else None
        self.calls = self.asked = self.requested = self.served = 0

    def _piece(self, nbytes):
        if self.policy == "whole":
            return nbytes
        if self.policy[0] == "fixed":
            return self.policy[1]
        return self.rng.randint(1, 4096)

    def __call__(self, nbytes):
        assert nbytes > 0
        self.calls += 1
        self.asked += nbytes
        self.requested = max(self.requested, self.served + nbytes)
        k = min(self._piece(nbytes), nbytes, self.end - self.served)
        piece = self.data[self.served:self.served + k]
        self.served += k
        return piece

    def drain(self, total, ask=lambda left: left):
        """what stream_impl's loop does for one chunk: ask for what is still missing until it is there or the stream ends"""
        out = b""
        while len(out) < total:
            piece = self(ask(total - len(out)))
            if not piece:
                break
            out += piece
        return out


POLICIES = ["whole", ("fixed", 7), ("random", 20261020)]


def zero_positions(n, chunk=CHUNK):
    """indices of the zero bases: the last index of chunk 0, the first of chunk 1 -- that one written as (0, 0) -- and
    the first of chunk 2"""
    return [i for i in (chunk - 1, chunk, 2 * chunk) if i < n and n > 1]


def patch_zero_record(data, index, rec_bytes):
    """the record at ``index`` as all-zero bytes: (0, 0), the other way a zero can stand in a file"""
    data = bytearray(data)
    data[index * rec_bytes:(index + 1) * rec_bytes] = bytes(rec_bytes)
    return bytes(data)


def oracle_bases(port, curve, group, n, first=8, chunk=CHUNK):
    bases = port.bases_seq(curve, group, n, first=first)
    for i in zero_positions(n, chunk):
        bases[i] = port.group_consts(curve, group)[1]
    return bases


def oracle_stream(port, curve, group, bases, chunk=CHUNK):
    """the uncompressed records of the bases; the zero at the first index of chunk 1 as (0, 0)"""
    rec = 2 * port.sizes(curve, group)["coord_bytes"]
    data = port.disk_write(curve, group, bases).tobytes()
    if bases.shape[0] > chunk:
        data = patch_zero_record(data, chunk, rec)
    return data, rec


def mnt_case(model, n, first=8, seed=5, chunk=CHUNK):
    """points (first + i + 1) G with the zeros of zero_positions, seeded scalars, and what their MSM is: every base is a
    multiple of G, so the sum is (sum k_i m_i mod r) G"""
    rng = random.Random(seed)
    pts, P = [], model.mul(first, model.one)
    for _ in range(n):
        P = model.add(P, model.one)
        pts.append(P)
    mult = [first + i + 1 for i in range(n)]
    for i in zero_positions(n, chunk):
        pts[i], mult[i] = mm.INF, 0
    ks = [rng.randrange(model.r) for _ in range(n)]
    return pts, ks, mult


def mnt_expect(model, ks, mult, n):
    return model.mul(sum(k * m for k, m in zip(ks[:n], mult[:n])) % model.r, model.one)


def mnt_stream(model, pts, chunk=CHUNK):
    rec = 2 * 8 * mm.WORDS * model.deg
    data = model.disk_write(pts)
    if len(pts) > chunk:
        data = patch_zero_record(data, chunk, rec)
    return data, rec


def mnt_precompute_points(model, pts, c, D):
    """[2^(j c)] P for j < D, base after base: the table multi_exp_stream_with_precompute reads"""
    out = []
    for P in pts:
        for _ in range(D):
            out.append(P)
            for _ in range(c):
                P = model.add(P, P)
    return out


# ---- the tiled file of the threaded reader
def tiled_scalars(r, block, copies, seed, first_neg=None):
    """a scalar of its own for every position of ``copies`` copies of a block of ``block`` records, as Python integers
    (copies, block), and the sum per block index mod r: an MSM over the tiled bases is the MSM over one block with these.
    first_neg: the copies from that one on hold the negated block, and their scalars count with a minus sign"""
    rng = random.Random(seed)
    ks = [[rng.randrange(r) for _ in range(block)] for _ in range(copies)]
    sign = [1 if first_neg is None or c < first_neg else -1 for c in range(copies)]
    summed = [sum(sign[c] * ks[c][i] for c in range(copies)) % r for i in range(block)]
    return ks, summed


def plain_records(ks, limbs):
    """integers as plain Fr records of ``limbs`` 64-bit words"""
    a = np.zeros((len(ks), limbs), dtype=np.uint64)
    for w in range(limbs):
        a[:, w] = [(k >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for k in ks]
    return a
