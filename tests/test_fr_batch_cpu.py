"""The batched Fr transforms and the one-call witness map without a device: the symbols and bindings, the batch plan
against its rules (vectors of a workgroup, workgroups of a pass, the workspace), every refusal of the five call entries
that needs no context -- given with a null context, so that nothing can have looked at one first; amdmsm_last_error(NULL)
names the argument -- and the integer model of the witness map against the identity that defines it."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm
import qap_witness_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amdmsm_fr_fft_batch", "amdmsm_fr_fft_batch_device", "amdmsm_plan_fr_fft_batch", "amdmsm_fr_domain_fft_batch_device",
         "amdmsm_fr_qap_witness_map", "amdmsm_fr_qap_witness_map_device", "amdmsm_plan_fr_qap_witness_map"]
BASE = 0x7f0000000000   # a device address, aligned to anything
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = dm.OK, dm.BAD_ARG, dm.UNSUPPORTED, dm.TOO_LARGE
LDS = 1 << 10           # records of a workgroup's tile


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    import libff_amd

    L = libff_amd.load_library()
    L.amdmsm_last_error.restype = ctypes.c_char_p
    L.amdmsm_last_error.argtypes = [ctypes.c_void_p]
    return L


def test_symbols_are_exported_declared_and_bound(lib):
    import libff_amd
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert libff_amd.plan_fr_fft_batch is e.plan_fr_fft_batch and libff_amd.plan_fr_qap_witness_map is e.plan_fr_qap_witness_map
    want = {
        "fr_fft_batch": ["curve", "values"],
        "fr_fft_batch_device": ["curve", "d_values", "n", "batch", "d_out", "in_stride", "out_stride"],
        "fr_domain_fft_batch_device": ["curve", "d_values", "m", "batch", "d_out", "in_stride", "out_stride"],
        "qap_witness_map": ["curve", "mat_a", "mat_b", "mat_c", "z", "m", "blind", "plain"],
        "qap_witness_map_device": ["curve", "mat_a", "mat_b", "mat_c", "d_z", "n_z", "m", "d_h", "blind", "plain", "stream"],
    }
    for name, head in want.items():
        params = list(inspect.signature(getattr(e.Engine, name)).parameters)[1:]
        assert params[:len(head)] == head, (name, params)
    sig = inspect.signature(e.Engine.fr_fft_batch_device).parameters
    assert sig["in_stride"].default is None and sig["out_stride"].default is None
    assert inspect.signature(e.Engine.qap_witness_map).parameters["blind"].default is None


@pytest.mark.parametrize("curve", [0, 4, 2])
def test_batch_plan(curve):
    import libff_amd

    rec = fm.field(curve).limbs * 8
    up = lambda x: (x + 255) // 256 * 256
    for log_n, batch, tile in [(0, 1, 0), (0, 17, 0), (1, 3, 0), (3, 17, 0), (4, 1024, 0), (6, 17, 0), (8, 5, 0), (9, 3, 8), (9, 3, 4),
                               (10, 3, 0), (12, 3, 4), (12, 3, 8), (12, 16, 0), (16, 3, 0), (20, 3, 0), (8, 1024, 0), (20, 256, 0)]:
        n = 1 << log_n
        p = libff_amd.plan_fr_fft_batch(curve, n, batch, tile)
        one = libff_amd.plan_fr_fft(curve, n, tile)
        V = LDS // n if n < LDS else 1
        assert p["vectors_per_workgroup"] == V, (n, batch)
        assert p["workgroups"] == ((batch + V - 1) // V if n < LDS else batch * n // LDS), (n, batch)
        assert p["workgroups"] <= 1 << 18
        assert p["passes"] == one["passes"] and p["tile_log2"] == one["tile_log2"] and p["launches"] == one["passes"]
        assert p["butterflies"] == batch * one["butterflies"]
        # one set of batch packed vectors in the place of the single plan's one vector, the tables once; in place a second
        # set where the passes are an odd number above one
        tables = one["workspace_bytes"] - up(n * rec)
        assert p["workspace_bytes"] == up(batch * n * rec) + tables, (n, batch)
        second = up(batch * n * rec) if one["passes"] > 1 and one["passes"] % 2 else 0
        assert p["workspace_bytes_in_place"] == p["workspace_bytes"] + second, (n, batch, tile)
    assert libff_amd.plan_fr_fft_batch(curve, 64, 0)["workgroups"] == 0
    assert libff_amd.plan_fr_fft_batch(curve, 0, 5)["launches"] == 0
    assert libff_amd.plan_fr_fft_batch(curve, 1 << 12, 3, 4)["passes"] == 3


def test_batch_plan_refusals(lib):
    out = (ctypes.c_size_t * 8)()
    sz = ctypes.c_size_t
    plan = lambda curve, n, batch, tile, o=out: lib.amdmsm_plan_fr_fft_batch(curve, sz(n), sz(batch), tile, o)
    assert plan(0, 64, 3, 0) == OK
    assert plan(9, 64, 3, 0) == UNSUPPORTED
    assert plan(0, 48, 3, 0) == BAD_ARG and plan(0, 64, 3, 3) == BAD_ARG and plan(0, 64, 3, 9) == BAD_ARG
    assert plan(0, 64, 3, 0, None) == BAD_ARG
    assert plan(0, 1 << 29, 1, 0) == TOO_LARGE and plan(0, 1 << 20, 257, 0) == TOO_LARGE and plan(0, 2, (1 << 27) + 1, 0) == TOO_LARGE
    assert plan(0, 1 << 20, 256, 0) == OK and plan(0, 1, 1 << 28, 0) == OK
    q = (ctypes.c_size_t * 6)()
    wm = lambda curve, m, o=q: lib.amdmsm_plan_fr_qap_witness_map(curve, sz(m), o)
    assert wm(0, 48) == OK and list(q)[:4] == [1, 48, 32, 16] and q[5] == 2 * 2
    assert wm(0, 64) == OK and list(q)[:4] == [0, 64, 64, 0] and q[5] == 2
    assert wm(0, 44) == BAD_ARG and wm(9, 48) == UNSUPPORTED and wm(0, (1 << 28) + 1) == TOO_LARGE and wm(0, 48, None) == BAD_ARG
    assert wm(5, (1 << 17) + 1) == UNSUPPORTED


@pytest.mark.parametrize("curve", [0, 4, 2])   # 8, 10 and 12 words: alignment to 16, 8 and 16 bytes
def test_refusals_without_a_context(lib, curve):
    f = fm.field(curve)
    rec = f.limbs * 8
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    o = ctypes.byref(_Opts(ctypes.sizeof(_Opts), 0, 0, 1, 1, 0, None))
    bad_o = ctypes.byref(_Opts(ctypes.sizeof(_Opts) - 4, 0, 0, 1, 1, 0, None))
    err = lambda: lib.amdmsm_last_error(None).decode()
    N, M, K = 8, 12, 3
    keep = [np.ascontiguousarray(f.records([x], True)[0]) for x in (f.root(N), f.root(4), fm.GENERATOR[curve], f.root(1 << 20))]
    wp, w4p, gp, w20p = (vp(a.ctypes.data) for a in keep)
    A, OUT = BASE, BASE + (1 << 20)
    host = np.ones((4 * K * M, f.limbs), dtype=np.uint64)
    hp = lambda k=0: vp(host.ctypes.data + k)

    def fft(n=N, batch=K, si=None, so=None, src=A, dst=OUT, omega=wp, tile=0, opts=o, curve=curve):
        return lib.amdmsm_fr_fft_batch_device(None, curve, vp(src), sz(n), sz(batch), sz(n if si is None else si),
                                              sz(n if so is None else so), omega, None, None, None, tile, opts, vp(dst))

    def hfft(n=N, batch=K, src=hp(), dst=hp(K * N * rec), omega=wp, tile=0, opts=o, curve=curve):
        return lib.amdmsm_fr_fft_batch(None, curve, src, sz(n), sz(batch), omega, None, None, None, tile, opts, dst)

    def dfft(m=M, batch=K, si=None, so=None, src=A, dst=OUT, flags=0, coset=None, tile=0, opts=o, curve=curve):
        return lib.amdmsm_fr_domain_fft_batch_device(None, curve, vp(src), sz(m), sz(batch), sz(m if si is None else si),
                                                     sz(m if so is None else so), flags, coset, tile, opts, vp(dst))

    blind = np.ascontiguousarray(f.records([1, 2, 3], True))
    over = blind.copy()
    over[1] = np.frombuffer(f.r.to_bytes(rec, "little"), dtype="<u8")
    bp, overp = vp(blind.ctypes.data), vp(over.ctypes.data)

    def wmap(m=48, z=A, n_z=10, h=OUT, bl=None, opts=o, curve=curve, host_entry=False):
        fn = lib.amdmsm_fr_qap_witness_map if host_entry else lib.amdmsm_fr_qap_witness_map_device
        return fn(None, curve, u64(1), u64(2), u64(3), vp(z), sz(n_z), sz(m), bl, opts, vp(h))

    cases = [
        # what the single-vector entry refuses, with its code and words
        (lambda: fft(n=6), BAD_ARG, "power of two"), (lambda: fft(n=1 << 29, batch=1), TOO_LARGE, "n ="),
        (lambda: fft(tile=3), BAD_ARG, "tile_log2"), (lambda: fft(src=0), BAD_ARG, "values"), (lambda: fft(dst=0), BAD_ARG, "output"),
        (lambda: fft(omega=None), BAD_ARG, "omega"), (lambda: fft(omega=w4p), BAD_ARG, "omega"),
        (lambda: fft(opts=bad_o), BAD_ARG, ""), (lambda: fft(curve=9), UNSUPPORTED, ""),
        (lambda: hfft(n=6), BAD_ARG, "power of two"), (lambda: hfft(src=None), BAD_ARG, "values"), (lambda: hfft(tile=9), BAD_ARG, "tile_log2"),
        (lambda: hfft(n=1 << 20, batch=257, omega=w20p), TOO_LARGE, "batch"), (lambda: hfft(curve=9), UNSUPPORTED, ""),
        # what the batch adds
        (lambda: fft(n=1 << 20, batch=257, omega=w20p), TOO_LARGE, "batch"),
        (lambda: fft(si=(1 << 64) // rec // 2 + 1), TOO_LARGE, "in_stride"), (lambda: fft(so=(1 << 64) // rec // 2 + 1), TOO_LARGE, "out_stride"),
        (lambda: fft(si=N - 1), BAD_ARG, "in_stride"), (lambda: fft(so=N - 1), BAD_ARG, "out_stride"),
        (lambda: fft(src=A + 4), BAD_ARG, "aligned"), (lambda: fft(dst=OUT + 4), BAD_ARG, "aligned"),
        (lambda: fft(dst=A + rec), BAD_ARG, "overlap"), (lambda: fft(dst=A + (K * N - 1) * rec), BAD_ARG, "overlap"),
        (lambda: fft(src=A + 2 * N * rec, dst=A, so=N + 1), BAD_ARG, "overlap"),      # the last output vector reaches the input
        (lambda: fft(dst=A, si=N + 2, so=N + 1), BAD_ARG, "overlap"),                  # one address, two strides
        (lambda: dfft(m=7), BAD_ARG, "domain size"), (lambda: dfft(m=(1 << 28) + 1, batch=1), TOO_LARGE, ""),
        (lambda: dfft(m=1 << 20, batch=257), TOO_LARGE, "batch"), (lambda: dfft(flags=2), BAD_ARG, "flags"),
        (lambda: dfft(src=0), BAD_ARG, "values"), (lambda: dfft(si=M - 1), BAD_ARG, "in_stride"), (lambda: dfft(so=M - 1), BAD_ARG, "out_stride"),
        (lambda: dfft(dst=A + rec), BAD_ARG, "overlap"), (lambda: dfft(dst=A, so=M + 1), BAD_ARG, "overlap"),
        (lambda: dfft(src=A + 4), BAD_ARG, "aligned"), (lambda: dfft(curve=9), UNSUPPORTED, ""), (lambda: dfft(opts=bad_o), BAD_ARG, ""),
        (lambda: dfft(m=(1 << 17) + 1, curve=5), UNSUPPORTED, "geometric"),
        # the witness map
        (lambda: wmap(m=44), BAD_ARG, "m = 44 is not a domain size"), (lambda: wmap(m=(1 << 28) + 1), TOO_LARGE, ""),
        (lambda: wmap(curve=9), UNSUPPORTED, ""), (lambda: wmap(m=(1 << 17) + 1, curve=5), UNSUPPORTED, "geometric"),
        (lambda: wmap(z=0), BAD_ARG, "d_z"), (lambda: wmap(h=0), BAD_ARG, "d_h"),
        (lambda: wmap(z=A + 4), BAD_ARG, "aligned"), (lambda: wmap(h=OUT + 4), BAD_ARG, "aligned"),
        (lambda: wmap(h=A + 9 * rec), BAD_ARG, "overlap"), (lambda: wmap(z=OUT + 48 * rec), BAD_ARG, "overlap"), (lambda: wmap(h=A), BAD_ARG, "overlap"),
        (lambda: wmap(bl=overp), BAD_ARG, "blind[1]"), (lambda: wmap(opts=bad_o), BAD_ARG, ""),
        (lambda: wmap(m=44, host_entry=True), BAD_ARG, "domain size"), (lambda: wmap(z=0, host_entry=True), BAD_ARG, "z"),
        (lambda: wmap(bl=overp, host_entry=True), BAD_ARG, "blind[1]"),
    ]
    for k, (call, code, words) in enumerate(cases):
        assert call() == code, k
        if words:
            assert words in err(), (k, err())
    # every rule kept: the missing context is what answers, and it leaves the last message alone
    last = err()
    kept = [fft(), fft(dst=A), fft(si=N + 3, so=N + 5), fft(dst=A, si=N + 2, so=N + 2), fft(dst=A + K * N * rec), fft(batch=0, src=0, dst=0),
            fft(n=0, src=0, dst=0, omega=None), fft(batch=1, si=0, so=0), fft(n=1 << 20, batch=256, omega=w20p, dst=A + (rec << 28)),
            hfft(), hfft(batch=0, src=None, dst=None),
            dfft(), dfft(dst=A), dfft(si=M + 1, so=M + 7), dfft(flags=1, coset=gp, tile=4), dfft(m=16), dfft(batch=0, src=0, dst=0),
            wmap(), wmap(bl=bp), wmap(m=64), wmap(n_z=0, z=0), wmap(h=A + 10 * rec), wmap(host_entry=True)]
    assert kept == [BAD_ARG] * len(kept) and err() == last
    assert (host == 1).all()


def _cases():
    for curve in (0, 4):
        for m in (6, 12, 16):
            for blind in (None, (0, 0, 0), (3, 5, 7), "random"):
                yield pytest.param(curve, m, blind, id=f"{fm.CURVES[curve]}-{m}-{blind if blind != 'random' else 'random'}")


@pytest.mark.parametrize("curve,m,blind", list(_cases()))
def test_model_satisfies_the_definition(curve, m, blind):
    f = fm.field(curve)
    n_rows = m - 1 if m != 16 else 16      # zero-filled to m, and a full domain
    a, b, c, z = qm.random_system(curve, n_rows, 5, seed=m)
    if blind == "random":
        blind = tuple(fm.random_vector(curve, 3, seed=77))
    h = qm.witness_map(curve, a, b, c, z, m, blind)
    assert len(h) == m + 1 and all(0 <= x < f.r for x in h)
    assert qm.identity_holds(curve, a, b, c, z, m, h, blind)
    if not blind or blind == (0, 0, 0):
        assert h[m - 1] == 0 and h[m] == 0
        assert h == qm.witness_map(curve, a, b, c, z, m, None)
    else:
        assert h[m] == blind[0] * blind[1] % f.r
        # a wrong coefficient breaks the identity: the check is not vacuous
        h[1] = (h[1] + 1) % f.r
        assert not qm.identity_holds(curve, a, b, c, z, m, h, blind)
