"""The evaluation domains over Fr without a device: the symbols, libfqfft's choice of a domain for every size, the
elements and the vanishing polynomial against the integer model, the generator against the reference's, the model's own
decomposition against Horner's rule, and every refusal of the domain entries that needs no context (the way
tests/test_fr_call_rules_cpu.py calls entries: the context is null, so a call that keeps every rule answers BAD_ARG as
well -- what is pinned is that nothing looks at the context or behind a device address first; what the refusals say is
checked with a context in tests/test_gpu_fr_domain.py)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import fr_domain_model as dm
import fr_fft_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amdmsm_fr_domain", "amdmsm_fr_domain_element", "amdmsm_fr_domain_vanishing", "amdmsm_fr_domain_z_terms",
         "amdmsm_fr_multiplicative_generator", "amdmsm_fr_domain_fft", "amdmsm_fr_domain_fft_device",
         "amdmsm_fr_domain_divide_by_z", "amdmsm_fr_domain_divide_by_z_device"]
SIX = list(fm.CURVES)
BASE = 0x7f0000000000   # a device address, aligned to anything


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    import libff_amd

    return libff_amd.load_library()


def test_symbols_are_exported_and_declared(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("AMDMSM_DOMAIN_BASIC_RADIX2", "AMDMSM_DOMAIN_STEP_RADIX2", "AMDMSM_DOMAIN_INVERSE"):
        assert name in header


def answer(curve, min_size):
    """fr_domain as the model's tuple"""
    import libff_amd

    try:
        d = libff_amd.fr_domain(curve, min_size)
    except libff_amd.AmdMsmError as err:
        return (err.code,) + (None,) * 5
    return 0, d["kind"], d["m"], d["B"], d["S"], d["omega_log2"]


@pytest.mark.parametrize("curve", SIX)
def test_choice_equals_the_model_for_every_small_size(curve):
    bad = [n for n in range(0, 4101) if answer(curve, n) != dm.choose(curve, n)]
    assert not bad, bad[:8]


@pytest.mark.parametrize("curve", SIX)
def test_choice_at_the_limits(curve):
    for n in ((1 << 27) + 1, (1 << 27) + (1 << 26), 1 << 28, (1 << 28) + 1, (1 << 16) + 1, 1 << 17, (1 << 17) + 1, 1 << 18):
        assert answer(curve, n) == dm.choose(curve, n), n
    assert dm.choose(curve, (1 << 28) + 1)[0] == dm.TOO_LARGE


def test_choice_limits_are_what_the_contract_names():
    assert dm.choose(0, (1 << 27) + 1) == (0, dm.STEP, (1 << 27) + 1, 1 << 27, 1, 28)
    assert dm.choose(0, (1 << 27) + (1 << 26))[1:5] == (dm.STEP, 3 << 26, 1 << 27, 1 << 26)
    assert dm.choose(0, 1 << 28)[:3] == (0, dm.BASIC, 1 << 28)
    assert dm.choose(5, (1 << 16) + 1)[:3] == (0, dm.STEP, (1 << 16) + 1) and dm.choose(5, 1 << 17)[:3] == (0, dm.BASIC, 1 << 17)
    assert dm.choose(5, (1 << 17) + 1)[0] == dm.UNSUPPORTED and dm.choose(5, 1 << 18)[0] == dm.UNSUPPORTED
    assert answer(5, (1 << 17) + 1)[0] == dm.UNSUPPORTED
    # a size that is no domain size moves up: 7 -> 8, 11 -> 12, 13 -> 16 (8 + 8), 21 -> 24
    assert [dm.choose(0, n)[2] for n in (7, 11, 13, 21)] == [8, 12, 16, 24]


@pytest.mark.parametrize("curve", SIX)
def test_generator_is_the_reference_s(curve):
    import libff_amd

    golden = np.load(os.path.join(ROOT, "tests", "golden", "fr_domain.npz"))
    want = int.from_bytes(np.ascontiguousarray(golden[fm.CURVES[curve] + "/multiplicative_generator"], dtype="<u8").tobytes(), "little")
    assert libff_amd.fr_multiplicative_generator(curve) == want == fm.GENERATOR[curve]
    f = fm.field(curve)
    mont = libff_amd.fr_multiplicative_generator(curve, plain=False)
    assert mont == want * f.R % f.r


@pytest.mark.parametrize("curve", [0, 4, 2])
def test_elements_and_vanishing_polynomial(curve):
    import libff_amd

    f = fm.field(curve)
    rng = random.Random(77 + curve)
    for m in (3, 5, 6, 12, 24, 40, 8):
        xs = [libff_amd.fr_domain_element(curve, m, j) for j in range(m)]
        assert xs == dm.elements(curve, m), m
        assert len(set(xs)) == m
        terms = libff_amd.fr_domain_z_terms(curve, m)
        assert terms == dm.z_terms(curve, m), m
        for x in xs:
            assert libff_amd.fr_domain_vanishing(curve, m, x) == 0
            assert sum(c * pow(x, i, f.r) for i, c in terms) % f.r == 0
        t = rng.randrange(f.r)
        assert libff_amd.fr_domain_vanishing(curve, m, t) == dm.vanishing(curve, m, t) != 0
        assert sum(c * pow(t, i, f.r) for i, c in terms) % f.r == dm.vanishing(curve, m, t)
        tm = t * f.R % f.r
        assert libff_amd.fr_domain_vanishing(curve, m, tm, plain=False) == dm.vanishing(curve, m, t) * f.R % f.r
    with pytest.raises(libff_amd.AmdMsmError):
        libff_amd.fr_domain_element(curve, 7, 0)
    with pytest.raises(libff_amd.AmdMsmError):
        libff_amd.fr_domain_element(curve, 6, 6)


@pytest.mark.parametrize("curve", [0, 5])
@pytest.mark.parametrize("m", [3, 5, 6, 12, 20, 24, 48, 68, 16])
def test_model_decomposition_equals_horner(curve, m):
    f = fm.field(curve)
    a = fm.random_vector(curve, m, seed=11)
    for g in (1, fm.GENERATOR[curve]):
        want = dm.transform_horner(curve, a, g)
        assert dm.transform(curve, a, g) == want
        assert dm.interpolate(curve, want, g) == a
    g = fm.GENERATOR[curve]
    q = dm.divide_by_z(curve, a, g)
    xs = dm.elements(curve, m)
    assert all(q[j] * dm.vanishing(curve, m, g * xs[j] % f.r) % f.r == a[j] for j in range(m))
    B, S = dm.shape(curve, m)
    assert dm.divide_by_z(curve, a, 1) is None and dm.divide_by_z(curve, a, f.root(2 * B if S else m)) is None


@pytest.mark.parametrize("curve", [0, 4, 2])   # 8, 10 and 12 words: alignment to 16, 8 and 16 bytes
def test_refusals_without_a_context(lib, curve):
    f = fm.field(curve)
    rec = f.limbs * 8
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    o = ctypes.byref(_Opts(ctypes.sizeof(_Opts), 0, 0, 1, 1, 0, None))
    bad_o = ctypes.byref(_Opts(ctypes.sizeof(_Opts) - 4, 0, 0, 1, 1, 0, None))
    M = 12
    g = np.ascontiguousarray(f.records([fm.GENERATOR[curve]], True)[0])
    w = np.ascontiguousarray(f.records([f.root(16)], True)[0])   # omega of the domain of 12 = 8 + 4: w^(2 B) = 1
    host = np.ones((3 * M, f.limbs), dtype=np.uint64)
    hp = lambda k=0: vp(host.ctypes.data + k)
    gp, wp = vp(g.ctypes.data), vp(w.ctypes.data)
    A, OUT = BASE, BASE + 4 * M * rec

    def fft(m, src, dst, flags=0, tile=0, opts=o, coset=None, curve=curve):
        return lib.amdmsm_fr_domain_fft_device(None, curve, vp(src), sz(m), flags, coset, tile, opts, vp(dst))

    def div(m, src, dst, coset=gp, opts=o, curve=curve):
        return lib.amdmsm_fr_domain_divide_by_z_device(None, curve, sz(m), vp(src), coset, opts, vp(dst))

    refused = [
        fft(7, A, OUT), fft(13, A, OUT), fft(1, A, OUT), fft(0, A, OUT), div(7, A, OUT), div(1, A, OUT),   # no domain size
        fft(M, 0, OUT), fft(M, A, 0), div(M, 0, OUT), div(M, A, 0), div(M, A, OUT, coset=None),             # null pointers
        fft(M, A + 4, OUT), fft(M, A, OUT + 4), div(M, A + 4, OUT), div(M, A, OUT + 4),                     # off the alignment
        fft(M, A, A + rec), fft(M, A + rec, A), fft(M, A, A + (M - 1) * rec), div(M, A, A + rec), div(M, A + rec, A),   # partial overlap
        fft(M, A, OUT, tile=3), fft(M, A, OUT, tile=9), fft(M, A, OUT, flags=2), fft(M, A, OUT, flags=-1),  # tile, flags
        fft(M, A, OUT, opts=bad_o), div(M, A, OUT, opts=bad_o),                                              # struct_size
        div(M, A, OUT, coset=wp), div(16, A, OUT, coset=wp),                                                 # g^(2B) = 1, g^m = 1
    ]
    assert refused == [dm.BAD_ARG] * len(refused)
    assert fft(M, A, OUT, curve=9) == dm.UNSUPPORTED and div(M, A, OUT, curve=9) == dm.UNSUPPORTED
    assert fft((1 << 28) + 1, A, OUT) == dm.TOO_LARGE and div((1 << 28) + 1, A, OUT) == dm.TOO_LARGE
    assert fft((1 << 17) + 1, A, OUT, curve=5) == dm.UNSUPPORTED and div((1 << 17) + 1, A, OUT, curve=5) == dm.UNSUPPORTED
    # every rule kept: the missing context is what answers
    kept = [fft(M, A, OUT), fft(M, A, A), fft(M, A, A + M * rec), fft(M, A, OUT, flags=1, coset=gp, tile=4), fft(16, A, OUT),
            div(M, A, OUT), div(M, A, A), div(16, A, A + 16 * rec)]
    assert kept == [dm.BAD_ARG] * len(kept)
    # the host entries take the caller's memory as it comes and stop at the missing context too, the arrays untouched
    before = host.copy()
    hosted = [
        lib.amdmsm_fr_domain_fft(None, curve, hp(4), sz(M), 0, gp, 0, o, hp(4 + rec)),
        lib.amdmsm_fr_domain_fft(None, curve, hp(), sz(7), 0, None, 0, o, hp()),
        lib.amdmsm_fr_domain_divide_by_z(None, curve, sz(M), hp(4), gp, o, hp(4 + rec)),
        lib.amdmsm_fr_domain_divide_by_z(None, curve, sz(M), hp(), wp, o, hp()),
    ]
    assert hosted == [dm.BAD_ARG] * len(hosted) and (host == before).all()
