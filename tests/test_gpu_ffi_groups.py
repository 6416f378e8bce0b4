"""The FFI entry points (include/libff_amd_ffi.h) for bls12_381 G1 / G2, MNT4-298 G1 / G2 and MNT6-298 G1, and the
loaded-bases calls for all eleven groups, on the device.

Expected bytes: for the MNT groups the reference's own, recorded in tests/golden/ffi_mnt.npz (and, for inputs the
fixture does not hold, the integer model of tests/mnt_model.py, which tests/test_ffi_groups_cpu.py ties to those
recordings); for bls12_381 the oracle's restatement of group_element_write and multi_exp, with the reference-generated
curve_points of golden.npz for the subgroup verdicts -- as test_gpu_parity.py::test_ffi_multiexp does for the other
pairing curves.  Every rejected call must leave its output buffer untouched."""
import ctypes
import random

import numpy as np
import pytest

import ffi_wire as fw
import mnt_model as mm
from common import GROUPS, golden

pytestmark = pytest.mark.gpu

ALL_GROUPS = GROUPS + [(name, curve, group) for name, (_, curve, group) in sorted(fw.MNT_GROUPS.items())]
assert len(ALL_GROUPS) == 11


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _call(fn, a, b, o):
    """any (buffer, buffer, out) FFI function: <g>_multiexp, <curve>_g1_add, <curve>_g1_mul"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    fn.restype = ctypes.c_bool
    return bool(fn(_vp(a), ctypes.c_size_t(a.size), _vp(b), ctypes.c_size_t(b.size), _vp(o), ctypes.c_size_t(o.size)))


def _loaded(lib, handle, first, sc, o):
    sc = np.ascontiguousarray(sc)
    lib.amdmsm_ffi_multiexp_loaded.restype = ctypes.c_bool
    return bool(lib.amdmsm_ffi_multiexp_loaded(ctypes.c_uint64(int(handle)), ctypes.c_size_t(first), _vp(sc),
                                               ctypes.c_size_t(sc.size), _vp(o), ctypes.c_size_t(o.size)))


def _sentinel(n):
    return np.full(n, 0xA5, dtype=np.uint8)


def _check_rejections(fn, bases_buf, sc_buf, E, fb, cb):
    """the three wrong sizes, a coordinate >= q, a flipped low bit of Y, a scalar >= r: false, output untouched"""
    for bad_b, bad_s, o in ((bases_buf[:-1], sc_buf, _sentinel(E)), (bases_buf, sc_buf[:-fb], _sentinel(E)),
                            (bases_buf, sc_buf, _sentinel(E - 1))):
        assert not _call(fn, bad_b, bad_s, o)
        assert (o == 0xA5).all()
    for mutate in ("range", "curve", "scalar"):
        b3, s3, o = bases_buf.copy(), sc_buf.copy(), _sentinel(E)
        if mutate == "range":
            b3[5 * E: 5 * E + cb] = 0xFF
        elif mutate == "curve":
            b3[7 * E + E - 1] ^= 1
        else:
            s3[3 * fb: 4 * fb] = 0xFF
        assert not _call(fn, b3, s3, o), mutate
        assert (o == 0xA5).all(), mutate


# ---------------------------------------------------------------------------------------------- bls12_381
@pytest.mark.parametrize("name,curve,group", [g for g in GROUPS if g[1] == 3])
def test_bls12_381_multiexp(engine, port, name, curve, group):
    fn = getattr(engine.lib, f"{name}_multiexp")
    n = {1: 300, 2: 120}[group]
    bases = port.bases_seq(curve, group, n, first=17)
    sc = port.scalars_sha512(curve, 900, n)
    s = port.sizes(curve, group)
    cb, fb = s["coord_bytes"], s["fr_bytes"]
    E = 2 * cb
    assert (fb, E) == (32, 96 * group)
    bases_buf = np.concatenate([port.ffi_group_write(curve, group, b) for b in bases])
    sc_buf = np.concatenate([port.ffi_fr_write(curve, x) for x in sc])
    want = port.ffi_group_write(curve, group, port.multi_exp(curve, group, bases, sc, port.BDLO12_SIGNED, 1))
    out = np.zeros(E, dtype=np.uint8)
    assert _call(fn, bases_buf, sc_buf, out)
    assert (out == want).all()
    # a zero base ((0, 1) encoding) is accepted and ignored
    zero_enc = port.ffi_group_write(curve, group, port.group_consts(curve, group)[1])
    b2 = bases_buf.copy()
    b2[:E] = zero_enc
    bz = bases.copy()
    bz[0] = port.group_consts(curve, group)[1]
    want2 = port.ffi_group_write(curve, group, port.multi_exp(curve, group, bz, sc, port.BDLO12_SIGNED, 1))
    assert _call(fn, b2, sc_buf, out) and (out == want2).all()
    _check_rejections(fn, bases_buf, sc_buf, E, fb, cb)
    # on the curve: accepted exactly where the reference's is_in_safe_subgroup() holds ([r]P == 0,
    # bls12_381_g1.cpp:335, bls12_381_g2.cpp:362)
    cp, flags = golden()[f"{name}/curve_points"], golden()[f"{name}/curve_points_flags"]
    assert cp.shape[0] > 0
    for k in range(cp.shape[0]):
        assert flags[k] & 1
        b4, o = bases_buf.copy(), _sentinel(E)
        b4[9 * E: 10 * E] = port.ffi_group_write(curve, group, cp[k])
        ok = _call(fn, b4, sc_buf, o)
        assert ok == bool(flags[k] & 2), (k, int(flags[k]))
        if ok:
            bb = bases.copy()
            bb[9] = cp[k]
            assert (o == port.ffi_group_write(curve, group, port.multi_exp(curve, group, bb, sc, port.BDLO12_SIGNED, 1))).all()
        else:
            assert (o == 0xA5).all()
    # empty input -> zero = (0, 1)
    assert _call(fn, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), out)
    assert (out == zero_enc).all()


def test_bls12_381_g1_add_mul(engine, port):
    """bls12_381_init / _g1_add / _g1_mul against the oracle's group law: P + Q, P + P, P + (-P), P + 0, 0 + Q, 0 + 0;
    s = random, 0, 1, r - 1; wrong sizes, a scalar >= r and an off-curve operand rejected."""
    curve, group = 3, 1
    lib = engine.lib
    lib.bls12_381_init.restype = ctypes.c_bool
    assert lib.bls12_381_init()
    add, mul = lib.bls12_381_g1_add, lib.bls12_381_g1_mul
    pts = port.bases_seq(curve, group, 6, first=40)
    zero = port.group_consts(curve, group)[1]
    enc = lambda p: port.ffi_group_write(curve, group, p)   # noqa: E731
    neg0 = port.group_op(curve, group, 3, pts[0])
    pairs = [(pts[0], pts[1]), (pts[2], pts[2]), (pts[0], neg0), (pts[4], zero), (zero, pts[5]), (zero, zero)]
    for k, (a, b) in enumerate(pairs):
        want = enc(port.group_op(curve, group, 4, port.group_op(curve, group, 5, a, b)))
        o = _sentinel(96)
        assert _call(add, enc(a), enc(b), o), k
        assert (o == want).all(), k
    assert (enc(port.group_op(curve, group, 4, port.group_op(curve, group, 5, pts[0], neg0))) == enc(zero)).all()
    r_int = sum(int(x) << (64 * i) for i, x in enumerate(golden()["bls12_381_g1/fr_modulus"]))
    be = lambda v: np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8).copy()   # noqa: E731
    rnd = port.scalars_sha512(curve, 4000, 1)[0]
    rnd_int = int.from_bytes(bytes(port.ffi_fr_write(curve, rnd)), "big")
    for k, v in enumerate((rnd_int, 0, 1, r_int - 1)):
        plain = np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)
        s_mont = port.fr_from_bigint(curve, plain.reshape(1, 4))
        want = enc(port.multi_exp(curve, group, pts[3:4], s_mont, port.BDLO12_SIGNED, 1))
        o = _sentinel(96)
        assert _call(mul, enc(pts[3]), be(v), o), k
        assert (o == want).all(), k
        if v == 1:
            assert (o == enc(pts[3])).all()
        if v == 0:
            assert (o == enc(zero)).all()
    o = _sentinel(96)
    assert not _call(mul, enc(pts[3]), be(r_int), o) and (o == 0xA5).all()
    off = enc(pts[2]).copy()
    off[-1] ^= 1
    assert not _call(add, off, enc(pts[1]), o) and (o == 0xA5).all()
    for fn, a, b in ((add, enc(pts[0]), enc(pts[1])), (mul, enc(pts[0]), be(5))):
        assert not _call(fn, a[:-1], b, o)
        assert not _call(fn, a, b[:-1], o)
        assert not _call(fn, a, b, o[:-1])
        assert (o == 0xA5).all()


# ---------------------------------------------------------------------------------------------- MNT4 / MNT6
@pytest.mark.parametrize("name", sorted(fw.MNT_GROUPS))
def test_mnt_multiexp(engine, name):
    C, curve, group = fw.MNT_GROUPS[name]
    f = fw.fixtures()
    fn = getattr(engine.lib, f"{name}_multiexp")
    E, fb, cb = fw.element_bytes(C), fw.FB, fw.FB * C.deg
    bases_rows, sc_rows = f[f"{name}/bases"], f[f"{name}/scalars"]
    bases_buf, sc_buf = np.ascontiguousarray(bases_rows).reshape(-1), np.ascontiguousarray(sc_rows).reshape(-1)
    out = np.zeros(E, dtype=np.uint8)
    assert _call(fn, bases_buf, sc_buf, out)
    assert (out == f[f"{name}/msm_out"]).all()   # what the reference's multi_exp and group_element_write gave
    # a zero base is accepted: the sum loses s_0 * B_0
    pts = [fw.decode_point(C, b) for b in bases_rows]
    ks = [fw.decode_scalar(s) for s in sc_rows]
    total = fw.decode_point(C, f[f"{name}/msm_out"])
    zero_enc = fw.encode_point(C, mm.INF)
    b2 = bases_buf.copy()
    b2[:E] = zero_enc
    assert _call(fn, b2, sc_buf, out)
    assert (out == fw.encode_point(C, C.add(total, C.neg(C.mul(ks[0], pts[0]))))).all()
    _check_rejections(fn, bases_buf, sc_buf, E, fb, cb)
    # the second Fq2 component is range-checked too
    if C.deg == 2:
        b3, o = bases_buf.copy(), _sentinel(E)
        b3[4 * E + fb: 4 * E + 2 * fb] = 0xFF
        assert not _call(fn, b3, sc_buf, o) and (o == 0xA5).all()
    # curve points: accepted or rejected exactly as the reference's group_element_read did
    cp, ok_ref = f[f"{name}/curve_points"], f[f"{name}/curve_points_ok"]
    for k in range(cp.shape[0]):
        b4, o = bases_buf.copy(), _sentinel(E)
        b4[9 * E: 10 * E] = cp[k]
        ok = _call(fn, b4, sc_buf, o)
        assert ok == bool(ok_ref[k]), k
        if ok:
            P = fw.decode_point(C, cp[k])
            want = C.add(C.add(total, C.neg(C.mul(ks[9], pts[9]))), C.mul(ks[9], P))
            assert (o == fw.encode_point(C, want)).all(), k
        else:
            assert (o == 0xA5).all(), k
    assert _call(fn, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), out)
    assert (out == zero_enc).all()


@pytest.mark.parametrize("name", sorted(fw.MNT_GROUPS))
def test_mnt_add_mul(engine, name):
    """Every recorded a + b and s * p row.  G1: through <curve>_init / _g1_add / _g1_mul; MNT4 G2 has no such entries
    (as in the reference's FFI), so its rows run as the MSMs those entries are: 1 * a + 1 * b and s * p."""
    C, curve, group = fw.MNT_GROUPS[name]
    f = fw.fixtures()
    lib = engine.lib
    E = fw.element_bytes(C)
    one = fw.encode_scalar(1)
    if group == 1:
        cname = name.split("_")[0]
        init, add, mul = (getattr(lib, f"{cname}_{x}") for x in ("init", "g1_add", "g1_mul"))
        init.restype = ctypes.c_bool
        assert init()
        do_add = lambda a, b, o: _call(add, a, b, o)   # noqa: E731
        do_mul = lambda p, s, o: _call(mul, p, s, o)   # noqa: E731
    else:
        msm = getattr(lib, f"{name}_multiexp")
        do_add = lambda a, b, o: _call(msm, np.concatenate([a, b]), np.concatenate([one, one]), o)   # noqa: E731
        do_mul = lambda p, s, o: _call(msm, p, s, o)   # noqa: E731
    A, B, O = (f[f"{name}/add_{x}"] for x in ("a", "b", "out"))
    for k in range(A.shape[0]):
        o = _sentinel(E)
        assert do_add(A[k], B[k], o), k
        assert (o == O[k]).all(), k
    P, S, O = (f[f"{name}/mul_{x}"] for x in ("p", "s", "out"))
    for k in range(P.shape[0]):
        o = _sentinel(E)
        assert do_mul(P[k], S[k], o), k
        assert (o == O[k]).all(), k
    # rejected operands leave the output alone
    o = _sentinel(E)
    assert not do_mul(P[0], fw.encode_scalar(C.r), o) and (o == 0xA5).all()
    off = A[0].copy()
    off[-1] ^= 1
    assert not do_add(off, B[0], o) and (o == 0xA5).all()
    if group == 1:
        for fn, a, b in ((add, A[0], B[0]), (mul, P[0], S[0])):
            assert not _call(fn, a[:-1], b, o)
            assert not _call(fn, a, b[:-1], o)
            assert not _call(fn, a, b, o[:-1])
            assert (o == 0xA5).all()


# ---------------------------------------------------------------------------------------------- loaded bases
def _inputs(port, name, curve, group, n):
    """(bases (n, E), scalars (n, fb), one curve point outside the safe subgroup or None) in the wire format"""
    if name in fw.MNT_GROUPS:
        C = fw.MNT_GROUPS[name][0]
        rng = random.Random(77 + curve * 2 + group)
        P, pts = C.mul(5, C.one), []
        for _ in range(n):
            pts.append(P)
            P = C.add(P, C.one)
        bases = np.stack([fw.encode_point(C, p) for p in pts])
        sc = np.stack([fw.encode_scalar(rng.randrange(C.r)) for _ in range(n)])
        f = fw.fixtures()
        bad = [f[f"{name}/curve_points"][k] for k in range(f[f"{name}/curve_points"].shape[0])
               if not f[f"{name}/curve_points_ok"][k]]
        return bases, sc, (bad[0] if bad else None)
    b = port.bases_seq(curve, group, n, first=23)
    s = port.scalars_sha512(curve, 1700, n)
    bases = np.stack([port.ffi_group_write(curve, group, x) for x in b])
    sc = np.stack([port.ffi_fr_write(curve, x) for x in s])
    cp, flags = golden()[f"{name}/curve_points"], golden()[f"{name}/curve_points_flags"]
    bad = [port.ffi_group_write(curve, group, cp[k]) for k in range(cp.shape[0]) if (flags[k] & 1) and not (flags[k] & 2)]
    return bases, sc, (bad[0] if bad else None)


def _check_loaded(engine, name, curve, group, bases, sc, outside, first):
    import libff_amd
    from libff_amd import ffi

    lib = engine.lib
    n, E = bases.shape
    fb = sc.shape[1]
    assert ffi.element_sizes(curve, group) == {"fr_bytes": fb, "element_bytes": E}
    one_shot = lambda lo, hi: ffi.multiexp(curve, group, bases[lo:hi].reshape(-1), sc[lo:hi].reshape(-1))   # noqa: E731
    whole = one_shot(0, n)
    assert whole is not None
    h = ffi.load_bases(curve, group, bases.reshape(-1))
    assert h is not None and int(h) != 0 and h.n == n
    ms = ffi.last_timings()   # of the load: upload, decode + validation, no MSM
    assert ms is not None and ms[0] >= 0 and ms[1] > 0 and ms[2] == 0
    # a second vector alive at the same time: the same points in reverse order
    rev = np.ascontiguousarray(bases[::-1])
    h2 = ffi.load_bases(curve, group, rev.reshape(-1))
    assert h2 is not None and int(h2) not in (0, int(h))
    assert ffi.multiexp_loaded(h, sc.reshape(-1)) == whole
    ms = ffi.last_timings()
    assert ms is not None and len(ms) == 3 and all(x >= 0 for x in ms)
    assert ffi.multiexp_loaded(h2, np.ascontiguousarray(sc[::-1]).reshape(-1)) == whole
    # a sub-range that does not start at point 0, on both handles
    m = n - first - 3
    part = one_shot(first, first + m)
    assert part is not None and part != whole
    assert ffi.multiexp_loaded(h, sc[first:first + m].reshape(-1), first_point=first) == part
    assert ffi.multiexp_loaded(h2, np.ascontiguousarray(sc[first:first + m][::-1]).reshape(-1),
                               first_point=n - first - m) == part
    assert ffi.multiexp_loaded(h, sc.reshape(-1)) == whole   # and the whole vector again
    # n = 0 -> (0, 1), at any admissible first point
    zero = ffi.multiexp(curve, group, b"", b"")
    assert zero is not None and ffi.multiexp_loaded(h, b"") == zero and ffi.multiexp_loaded(h, b"", first_point=n) == zero
    # rejected, output untouched: range past the end, ragged scalar size, scalar >= r, wrong output size, unknown handle
    o = _sentinel(E)
    assert not _loaded(lib, h, 1, sc.reshape(-1), o)
    assert not _loaded(lib, h, n + 1, sc[:0].reshape(-1), o)
    assert not _loaded(lib, h, 2 ** 63, sc[:2].reshape(-1), o)
    assert not _loaded(lib, h, 0, sc.reshape(-1)[:-1], o)
    big = sc.copy()
    big[3] = 0xFF
    assert not _loaded(lib, h, 0, big.reshape(-1), o)
    assert not _loaded(lib, h, 0, sc.reshape(-1), o[:-1])
    assert not _loaded(lib, int(h2) + 1000, 0, sc.reshape(-1), o)
    assert not _loaded(lib, 0, 0, sc.reshape(-1), o)
    assert (o == 0xA5).all()
    assert ffi.multiexp_loaded(h, sc.reshape(-1), first_point=1) is None
    # loads that must fail and leave the handle unwritten: ragged size, off-curve point, point outside the subgroup
    lib.amdmsm_ffi_bases_load.restype = ctypes.c_bool
    for case in ("size", "curve", "subgroup"):
        b = bases.copy()
        if case == "curve":
            b[n // 2, E - 1] ^= 1
        elif case == "subgroup":
            if outside is None:   # cofactor 1: every curve point is in the group
                continue
            b[n // 3] = outside
        flat = np.ascontiguousarray(b).reshape(-1)
        if case == "size":
            flat = np.ascontiguousarray(flat[:-1])
        hv = ctypes.c_uint64(0xDEADBEEF)
        assert not lib.amdmsm_ffi_bases_load(curve, group, _vp(flat), ctypes.c_size_t(flat.size), ctypes.byref(hv)), case
        assert hv.value == 0xDEADBEEF, case
        assert ffi.load_bases(curve, group, flat) is None, case
    with pytest.raises(libff_amd.AmdMsmError):
        ffi.load_bases(libff_amd.MNT6, 2, bases.reshape(-1))
    # freeing one handle leaves the other usable; a freed handle fails; a second free fails
    assert ffi.free_bases(h) is True
    o = _sentinel(E)
    assert not _loaded(lib, h, 0, sc.reshape(-1), o) and (o == 0xA5).all()
    assert ffi.multiexp_loaded(h, sc.reshape(-1)) is None
    assert ffi.free_bases(h) is None
    assert ffi.multiexp_loaded(h2, np.ascontiguousarray(sc[::-1]).reshape(-1)) == whole
    assert ffi.free_bases(h2) is True
    assert ffi.free_bases(h2) is None


@pytest.mark.parametrize("name,curve,group", ALL_GROUPS, ids=[g[0] for g in ALL_GROUPS])
def test_loaded_bases(engine, port, name, curve, group):
    bases, sc, outside = _inputs(port, name, curve, group, 100)
    if name not in ("alt_bn128_g1", "mnt4_g1", "mnt6_g1"):
        assert outside is not None
    _check_loaded(engine, name, curve, group, bases, sc, outside, first=37)


def test_loaded_bases_2p16(engine, port):
    """bls12_377 G1 at 2^16 points: bases (5 + i) G made on the device and written in the wire format, scalars below
    2^248 < r."""
    import libff_amd

    curve, group, n = libff_amd.BLS12_377, 1, 1 << 16
    fl = libff_amd.sizes(curve, group)["affine_bytes"] // 16
    am = np.ascontiguousarray(engine.gen_bases_seq(curve, group, n, first=5)[:, : 2 * fl]).reshape(2 * n, fl)
    one = np.zeros_like(am)
    one[:, 0] = 1
    plain = engine.field_op(curve, group, 0, am, one)   # Montgomery product with the integer 1: the plain value
    bases = np.ascontiguousarray(np.ascontiguousarray(plain[:, ::-1]).view(np.uint8).reshape(2 * n, fl, 8)[..., ::-1])
    bases = bases.reshape(n, 2 * fl * 8)
    # the first points agree with the oracle's encoding of the same multiples of G
    want = port.bases_seq(curve, group, 4, first=5)
    for k in range(4):
        assert (bases[k] == port.ffi_group_write(curve, group, want[k])).all(), k
    sc = np.random.default_rng(2024).integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 0] = 0
    outside = _inputs(port, "bls12_377_g1", curve, group, 1)[2]
    _check_loaded(engine, "bls12_377_g1", curve, group, bases, sc, outside, first=12345)
