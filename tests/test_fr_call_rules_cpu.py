"""The rules for vectors in device memory (alignment, partial overlap, a one-record result inside a vector) are stated
once in the engine and used by every Fr entry that takes such a vector.  No GPU and no context: the addresses are numbers
that nothing reads, every refusal is BAD_ARG, and a call that keeps every rule gets as far as the missing context --
which answers BAD_ARG as well, so what this pins is that no entry looks at the context, or at memory behind a device
address, before its rules hold.  What each refusal says is checked with a context in tests/test_gpu_fr_*.py."""
import ctypes

import numpy as np
import pytest

import fr_fft_model as model

BAD_ARG = -2
BASE = 0x7f0000000000   # a device address, aligned to anything
N = 8


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    import libff_amd

    return libff_amd.load_library()


@pytest.mark.parametrize("curve", [0, 4, 2])   # 8, 10 and 12 words: alignment to 16, 8 and 16 bytes
def test_device_vector_rules_without_a_context(lib, curve):
    f = model.field(curve)
    rec = f.limbs * 8
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    o = ctypes.byref(_Opts(ctypes.sizeof(_Opts), 0, 0, 1, 1, 0, None))
    w = np.ascontiguousarray(f.records([f.root(N)], True)[0])   # plain, as the options say
    host = np.ones((3 * N, f.limbs), dtype=np.uint64)
    hp = lambda k=0: vp(host.ctypes.data + k)
    wp = vp(w.ctypes.data)
    A, B, C, OUT, TOT = (BASE + i * 4 * N * rec for i in range(5))   # five vectors far apart

    fft = lambda n, src, dst: lib.amdmsm_fr_fft_device(None, curve, vp(src), sz(n), wp, None, None, None, 0, o, vp(dst))
    powers = lambda n, dst: lib.amdmsm_fr_powers_device(None, curve, wp, sz(n), o, vp(dst))
    muladd = lambda n, a, b, c, dst: lib.amdmsm_fr_muladd_device(None, curve, sz(n), vp(a), vp(b), vp(c), None, o, vp(dst))
    apply = lambda x, dst: lib.amdmsm_fr_matrix_apply_device(None, ctypes.c_uint64(1), vp(x), sz(N), vp(dst), sz(N), o)
    scan = lambda n, a, b, dst, tot: lib.amdmsm_fr_scan_device(None, curve, sz(n), vp(a), None, vp(b), None, 0, 0, o, vp(dst), vp(tot))
    invert = lambda n, v, dst, cnt: lib.amdmsm_fr_batch_invert_device(None, curve, sz(n), vp(v), 0, o, vp(dst), vp(cnt))

    refused = [
        # a vector off its alignment, operand by operand
        fft(N, A + 4, OUT), fft(N, A, OUT + 4), powers(N, OUT + 4),
        muladd(N, A + 4, B, C, OUT), muladd(N, A, B + 4, C, OUT), muladd(N, A, B, C + 4, OUT), muladd(N, A, B, C, OUT + 4),
        apply(A + 4, OUT), apply(A, OUT + 4),
        scan(N, A + 4, B, OUT, TOT), scan(N, A, B + 4, OUT, TOT), scan(N, A, B, OUT + 4, TOT), scan(N, A, B, OUT, TOT + 4),
        invert(N, A + 4, OUT, TOT), invert(N, A, OUT + 4, TOT), invert(N, A, OUT, TOT + 4),
        # two vectors that share bytes without being one vector -- and for the matrix, being one
        fft(N, A, A + rec), fft(N, A + rec, A), apply(A, A + rec), apply(A + rec, A), apply(A, A),
        scan(N, A, B, A + rec, TOT), scan(N, A, B, B + (N - 1) * rec, TOT), scan(N, 0, B, B - rec, TOT),
        invert(N, A, A + rec, TOT), invert(N, A + rec, A, 0),
        # a one-record result inside a vector: its first bytes, its last, and the vector that is written
        scan(N, A, B, OUT, A), scan(N, A, B, OUT, B + (N - 1) * rec), scan(N, A, 0, A, A + 2 * rec), scan(N, A, B, OUT, OUT + rec),
        invert(N, A, OUT, A + 8), invert(N, A, OUT, OUT + N * rec - 8), invert(N, A, A, A),
    ]
    assert refused == [BAD_ARG] * len(refused)
    # every rule kept: vectors next to each other, in place, a result right behind a vector, absent operands, and nothing
    # of this at n = 0 -- the missing context is what answers, or nothing does
    kept = [
        fft(N, A, A), fft(N, A, A + N * rec), fft(0, 0, 0), fft(0, A + 4, A + 5), powers(N, OUT), powers(0, OUT + 4),
        muladd(N, A, B, 0, A), muladd(N, A, A + rec, C, OUT), muladd(0, A + 4, B, C, OUT),
        scan(N, A, B, A, A + N * rec), scan(N, A, B, B, 0), scan(N, 0, B, B + N * rec, TOT), scan(0, A + 4, B, A + 5, TOT),
        scan(0, A, B, OUT, A),
        invert(N, A, A, A + N * rec), invert(N, A, A + N * rec, A - 8), invert(0, A + 4, A + 5, TOT), invert(0, A, OUT, A),
    ]
    assert kept == [BAD_ARG] * len(kept)
    # the host entries take the caller's memory as it comes -- no alignment, overlap is the caller's affair -- and stop at
    # the missing context too; none of them has touched the arrays
    before = host.copy()
    hosted = [
        lib.amdmsm_fr_fft(None, curve, hp(4), sz(N), wp, None, None, None, 0, o, hp(4 + rec)),
        lib.amdmsm_fr_matrix_apply(None, ctypes.c_uint64(1), hp(4), sz(N), hp(4 + rec), sz(N), o),
        lib.amdmsm_fr_scan(None, curve, sz(N), hp(4), None, hp(4 + rec), None, 0, 0, o, hp(4 + 2 * rec), hp(4)),
        lib.amdmsm_fr_batch_invert(None, curve, sz(N), hp(4), o, hp(4 + rec), hp(12)),
        lib.amdmsm_fr_fft(None, curve, None, sz(0), None, None, None, None, 0, o, None),
        lib.amdmsm_fr_scan(None, curve, sz(0), None, None, hp(), None, 0, 0, o, None, hp()),
        lib.amdmsm_fr_batch_invert(None, curve, sz(0), None, o, None, None),
    ]
    assert hosted == [BAD_ARG] * len(hosted) and (host == before).all()
