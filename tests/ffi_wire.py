"""libff's FFI wire format (ffi/ffi_serialization.tcc) over tests/mnt_model.py's integer model of the MNT groups, and
the fixtures of tests/golden/ffi_mnt.npz: big-endian plain 40-byte integers, affine X || Y, Fq2 coordinates c1 then
c0, zero = (0, 1)."""
import os

import numpy as np

import mnt_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))
FB = 40   # bytes of one Fq / Fr element of MNT4-298 / MNT6-298 (bigint<5>)
# fixture group -> (model curve, engine curve id, engine group id)
MNT_GROUPS = {"mnt4_g1": (mm.MNT4, 4, 1), "mnt4_g2": (mm.MNT4_G2, 4, 2), "mnt6_g1": (mm.MNT6, 5, 1)}

_fix = None


def fixtures():
    global _fix
    if _fix is None:
        _fix = dict(np.load(os.path.join(HERE, "golden", "ffi_mnt.npz")))
    return _fix


def element_bytes(C):
    return 2 * FB * C.deg


def _coord(C, b):
    cs = [int.from_bytes(bytes(b[i * FB:(i + 1) * FB]), "big") for i in range(C.deg)]
    assert all(c < C.p for c in cs)
    return cs[0] if C.deg == 1 else (cs[1], cs[0])   # written c1 then c0


def decode_point(C, b):
    """wire bytes -> affine model point (None = zero); the coordinates must be in range"""
    b = np.asarray(b, dtype=np.uint8)
    assert b.size == element_bytes(C)
    x, y = _coord(C, b[:FB * C.deg]), _coord(C, b[FB * C.deg:])
    if x == C.F.zero() and y == (1 if C.deg == 1 else (1, 0)):
        return mm.INF
    return (x, y)


def encode_point(C, P):
    if P is mm.INF:
        P = (C.F.zero(), 1 if C.deg == 1 else (1, 0))
    out = b""
    for v in P:
        for c in reversed(C.F.comps(v)):
            out += int(c).to_bytes(FB, "big")
    return np.frombuffer(out, dtype=np.uint8).copy()


def decode_scalar(b):
    return int.from_bytes(bytes(np.asarray(b, dtype=np.uint8)), "big")


def encode_scalar(k):
    return np.frombuffer(int(k).to_bytes(FB, "big"), dtype=np.uint8).copy()


def mul_plain(C, k, P):
    """[k]P without reducing k modulo r (Curve.mul reduces, which would make [r]P trivially zero)"""
    R = mm.INF
    for bit in bin(k)[2:]:
        R = C.add(R, R)
        if bit == "1":
            R = C.add(R, P)
    return R


def in_subgroup(C, P):
    return mul_plain(C, C.r, P) is mm.INF
