"""The FFT over Fr scalars (amdmsm_fr_fft / _device, amdmsm_plan_fr_fft, amdmsm_fr_root_of_unity, amdmsm_fr_powers_device,
amdmsm_fr_muladd_device) as far as a host without a GPU can see it: the symbols are exported and declared, the Python
layer has the methods, the roots of unity are the reference's (tests/golden/fr_domain.npz), the plan counts passes, the
argument rules that need no device answer before the context is looked at, and the integer model of the GPU tests agrees
with itself."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import fr_fft_model as model
from common import to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_fr_fft", "amdmsm_fr_fft_device", "amdmsm_plan_fr_fft", "amdmsm_fr_root_of_unity", "amdmsm_fr_powers_device",
         "amdmsm_fr_muladd_device")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
CURVES = sorted(model.CURVES)


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


@pytest.fixture(scope="module")
def domain():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "fr_domain.npz")))


def test_the_symbols_are_exported_and_declared(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header
    assert "#define AMDMSM_ABI_VERSION 3" in header


def test_python_layer_has_the_methods():
    import libff_amd

    host = inspect.signature(libff_amd.Engine.fr_fft).parameters
    assert list(host)[:8] == ["self", "curve", "values", "omega", "inverse", "coset", "plain", "tile_log2"]
    assert host["omega"].default is None and host["inverse"].default is False and host["coset"].default is None
    assert host["plain"].default is False and host["tile_log2"].default == 0
    for name in ("fr_fft_device", "fr_powers_device", "fr_muladd_device"):
        assert callable(getattr(libff_amd.Engine, name)), name
    for name in ("plan_fr_fft", "fr_root_of_unity"):
        assert name in libff_amd.__all__ and callable(getattr(libff_amd, name)), name
    assert list(inspect.signature(libff_amd.plan_fr_fft).parameters) == ["curve", "n", "tile_log2"]
    assert list(inspect.signature(libff_amd.fr_root_of_unity).parameters) == ["curve", "n"]


@pytest.mark.parametrize("curve", CURVES)
def test_roots_of_unity_are_the_reference_s(lib, domain, curve):
    from libff_amd import fr_modulus, fr_root_of_unity, sizes

    name = model.CURVES[curve]
    s = int(domain[f"{name}/s"][0])
    r = fr_modulus(curve, 1)
    assert s == model.TWO_ADICITY[curve] and to_int(domain[f"{name}/multiplicative_generator"]) == model.GENERATOR[curve]
    assert to_int(domain[f"{name}/root_of_unity"]) == to_int(domain[f"{name}/root_s"])
    buf = (ctypes.c_uint8 * sizes(curve, 1)["fr_bytes"])()
    for k, key in ((1, "root_1"), (4, "root_4"), (s, "root_s")):
        want = to_int(domain[f"{name}/{key}"])
        assert fr_root_of_unity(curve, 1 << k) == want, k
        assert lib.amdmsm_fr_root_of_unity(curve, k, buf) == OK and int.from_bytes(bytes(buf), "little") == want
        assert pow(want, 1 << (k - 1), r) == r - 1
        assert model.field(curve).root(1 << k) == want
    assert fr_root_of_unity(curve, 1) == 1
    assert lib.amdmsm_fr_root_of_unity(curve, s + 1, buf) == BAD_ARG
    assert lib.amdmsm_fr_root_of_unity(curve, -1, buf) == BAD_ARG
    assert lib.amdmsm_fr_root_of_unity(curve, 4, None) == BAD_ARG
    with pytest.raises(ValueError):
        fr_root_of_unity(curve, 1 << (s + 1))
    with pytest.raises(ValueError):
        fr_root_of_unity(curve, 12)
    assert lib.amdmsm_fr_root_of_unity(6, 4, buf) == UNSUPPORTED


@pytest.mark.parametrize("curve", CURVES)
def test_plan_counts_passes(lib, curve):
    from libff_amd import plan_fr_fft, sizes

    rec = sizes(curve, 1)["fr_bytes"]
    base = plan_fr_fft(curve, 1)
    T, lo, hi = base["tile_log2"], base["tile_min"], base["tile_max"]
    assert lo <= T <= hi
    for tile in [0] + list(range(lo, hi + 1)):
        t = tile or T
        for lg in (0, 1, 2, t - 1, t, t + 1, 2 * t, 2 * t + 1, 3 * t + 1, 20, 28):
            p = plan_fr_fft(curve, 1 << lg, tile)
            assert p["tile_log2"] == t and (p["tile_min"], p["tile_max"]) == (lo, hi)
            assert p["passes"] == max(1, -(-lg // t)), (tile, lg)
            assert p["butterflies"] == (1 << lg) // 2 * lg
            assert p["workspace_bytes"] >= (1 << lg) * rec     # the vector the passes alternate with
            # and the powers of pre and post of the first and the last pass, each vector rounded up to 256 bytes
            first, last = min(t, lg), lg - (p["passes"] - 1) * t
            powers = ((1 << lg) >> first) + (1 << first) + ((1 << lg) >> last) + (1 << last)
            assert p["workspace_bytes"] <= ((1 << lg) + powers) * rec + 5 * 255
    out = (ctypes.c_size_t * 6)()
    for n in (3, 6, 1025):
        assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(n), 0, out) == BAD_ARG
    assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(1 << 29), 0, out) == TOO_LARGE
    assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(1 << 28), 0, out) == OK
    assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(8), lo - 1, out) == BAD_ARG
    assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(8), hi + 1, out) == BAD_ARG
    assert lib.amdmsm_plan_fr_fft(curve, ctypes.c_size_t(8), 0, None) == BAD_ARG
    assert lib.amdmsm_plan_fr_fft(6, ctypes.c_size_t(8), 0, out) == UNSUPPORTED


@pytest.mark.parametrize("curve", CURVES)
def test_refusals_that_need_no_device(lib, curve):
    """Without a context only the codes that differ from the missing context's own BAD_ARG can be told apart: too large
    and unknown curve, which are answered before the context is looked at.  The BAD_ARG refusals, with what
    amdmsm_last_error says of each, are in tests/test_gpu_fr_fft.py, where there is a context."""
    f = model.field(curve)
    n = 8
    vals = f.records(model.random_vector(curve, n), plain=False)
    out = np.full_like(vals, 0x5a5a5a5a5a5a5a5a)
    w = f.records([f.root(n)], plain=False)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def host(c, m):
        return lib.amdmsm_fr_fft(None, c, ptr(vals), ctypes.c_size_t(m), ptr(w), None, None, None, 0, None, ptr(out))

    def dev(c, m):
        return lib.amdmsm_fr_fft_device(None, c, ptr(vals), ctypes.c_size_t(m), ptr(w), None, None, None, 0, None, ptr(out))

    for call in (host, dev):
        assert call(curve, 1 << 29) == TOO_LARGE
        assert call(6, n) == UNSUPPORTED and call(-1, n) == UNSUPPORTED
        assert call(curve, n) == BAD_ARG     # every rule holds: the missing context is what is left to refuse
    z = ctypes.c_size_t(0)
    assert lib.amdmsm_fr_powers_device(None, 6, None, z, None, None) == UNSUPPORTED
    assert lib.amdmsm_fr_muladd_device(None, 6, z, None, None, None, None, None, None) == UNSUPPORTED
    assert lib.amdmsm_fr_powers_device(None, curve, ptr(w), ctypes.c_size_t((1 << 32) + 1), None, ptr(out)) == TOO_LARGE
    assert (out == 0x5a5a5a5a5a5a5a5a).all()


@pytest.mark.parametrize("curve", [0, 4, 2])
def test_model_recursion_equals_the_definition(lib, curve):
    f = model.field(curve)
    n = 16
    a, w = model.random_vector(curve, n), f.root(n)
    g = model.GENERATOR[curve]
    ninv, ginv, winv = pow(n, -1, f.r), pow(g, -1, f.r), pow(w, -1, f.r)
    assert model.fft(a, w, f.r) == model.naive(a, w, f.r)
    assert model.fft(a, w, f.r, pre=g) == model.naive(a, w, f.r, pre=g)
    assert model.fft(a, w, f.r, pre=3, post=5, scale=7) == model.naive(a, w, f.r, pre=3, post=5, scale=7)
    assert model.fft(model.fft(a, w, f.r), winv, f.r, scale=ninv) == a
    assert model.fft(model.fft(a, w, f.r, pre=g), winv, f.r, post=ginv, scale=ninv) == a
    assert model.fft([5], 1, f.r, scale=3) == [15] and model.fft([], 1, f.r) == []
    for plain in (False, True):
        assert f.ints(f.records(a, plain), plain) == a
    assert to_int(f.records([1], plain=False)[0]) == f.R % f.r
