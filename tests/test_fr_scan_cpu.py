"""The scans and the batch inversion over Fr (amdmsm_fr_scan / _device, amdmsm_fr_batch_invert / _device,
amdmsm_plan_fr_scan, amdmsm_fr_inverse) as far as a host without a GPU can see them: the symbols are exported and
declared, the Python layer has the methods, the host inversion agrees with Python's pow for the six fields in both
record forms, the plan entry reports the arithmetic of the integer model at n around every edge, every refusal that
needs no device is a refusal, the model agrees with itself, and the index arithmetic of the kernels runs clean under the
host compiler's sanitizers (tools/fr_scan_layout_check.cpp, a program of its own)."""
import ctypes
import inspect
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import fr_scan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_fr_scan", "amdmsm_fr_scan_device", "amdmsm_fr_batch_invert", "amdmsm_fr_batch_invert_device",
         "amdmsm_plan_fr_scan", "amdmsm_fr_inverse")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
CURVES = sorted(model.CURVES)
KIND_A, KIND_B, KIND_INVERT, REVERSE, EXCLUSIVE = 0x100, 0x200, 0x400, 1, 2


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def test_the_symbols_are_exported_and_declared(lib):
    import libff_amd.engine as e

    header = open(os.path.join(ROOT, "include", "amdmsm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS
        assert f"int {name}(" in header
    assert "#define AMDMSM_ABI_VERSION 3" in header
    for name, value in (("AMDMSM_SCAN_REVERSE", 1), ("AMDMSM_SCAN_EXCLUSIVE", 2), ("AMDMSM_SCAN_KIND_A", "0x100"),
                        ("AMDMSM_SCAN_KIND_B", "0x200"), ("AMDMSM_SCAN_KIND_INVERT", "0x400")):
        assert f"#define {name} {value}" in header
    assert (e.SCAN_REVERSE, e.SCAN_EXCLUSIVE, e.SCAN_KIND_A, e.SCAN_KIND_B, e.SCAN_KIND_INVERT) == (1, 2, 0x100, 0x200, 0x400)
    assert "has no Fr inversion" not in " ".join(header.split())


def test_python_layer_has_the_methods():
    import libff_amd

    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(libff_amd.plan_fr_scan) == ["curve", "n", "a", "b", "invert", "reverse", "exclusive", "tile_log2"]
    assert sig(libff_amd.fr_inverse) == ["curve", "x", "plain"]
    assert sig(libff_amd.Engine.fr_scan)[:4] == ["self", "curve", "a", "b"]
    assert sig(libff_amd.Engine.fr_scan_device)[:6] == ["self", "curve", "n", "d_out", "d_a", "d_b"]
    for method in (libff_amd.Engine.fr_scan, libff_amd.Engine.fr_scan_device):
        for word in ("a_const", "init", "reverse", "exclusive", "plain", "tile_log2"):
            assert word in sig(method), (method, word)
    assert sig(libff_amd.Engine.fr_batch_invert) == ["self", "curve", "values", "plain"]
    assert sig(libff_amd.Engine.fr_batch_invert_device) == ["self", "curve", "n", "d_values", "d_out", "d_zero_count", "plain",
                                                           "tile_log2", "stream"]
    for name in ("plan_fr_scan", "fr_inverse", "SCAN_REVERSE", "SCAN_EXCLUSIVE"):
        assert name in libff_amd.__all__


def test_the_model_agrees_with_itself():
    rng = random.Random(1)
    for curve in CURVES:
        r = model.field(curve).r
        n = 9
        a, b = [rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(n)]
        # a reverse scan is the forward scan of the reversed vectors
        for excl in (False, True):
            fwd, t1 = model.scan(r, n, a[::-1], b[::-1], init=5, exclusive=excl)
            rev, t2 = model.scan(r, n, a, b, init=5, reverse=True, exclusive=excl)
            assert fwd[::-1] == rev and t1 == t2
        # exclusive is inclusive moved by one, with init in front
        inc, total = model.scan(r, n, a, b, init=7)
        exc, total2 = model.scan(r, n, a, b, init=7, exclusive=True)
        assert exc == [7] + inc[:-1] and total == total2 == inc[-1]
        # prefix products, prefix sums, defaults of init
        prod, _ = model.scan(r, n, a)
        assert prod[3] == a[0] * a[1] * a[2] * a[3] % r
        sums, _ = model.scan(r, n, None, b)
        assert sums[4] == sum(b[:5]) % r
        assert model.scan(r, 0, a=[], init=None) == ([], 1) and model.scan(r, 0, b=[], init=None) == ([], 0)
        # synthetic division
        z = rng.randrange(r)
        q, pz = model.scan(r, n, None, b, a_const=z, init=0, reverse=True, exclusive=True)
        assert model.synthetic_division_holds(r, b, z, q, pz)
        assert not model.synthetic_division_holds(r, b, z, q, (pz + 1) % r)
        # inversion
        inv, zeros = model.invert(r, [0, 1, r - 1, a[0], 0])
        assert zeros == 2 and inv[0] == inv[4] == 0 and inv[1] == 1 and inv[2] == r - 1 and inv[3] * a[0] % r == 1


def _rec(v, limbs):
    return np.frombuffer(int(v).to_bytes(8 * limbs, "little"), dtype="<u8").astype(np.uint64)


def _int(rec):
    return int.from_bytes(np.ascontiguousarray(rec, dtype="<u8").tobytes(), "little")


@pytest.mark.parametrize("curve", CURVES)
def test_host_inverse_against_pow(lib, curve):
    import libff_amd

    f = model.field(curve)
    r, R = f.r, f.R
    rng = random.Random(curve)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for x in [1, 2, r - 1, r - 2, (r + 1) // 2] + [rng.randrange(1, r) for _ in range(5)]:
        want = pow(x, r - 2, r)
        assert want * x % r == 1
        assert libff_amd.fr_inverse(curve, x) == want
        assert libff_amd.fr_inverse(curve, x * R % r, plain=False) == want * R % r
    for plain in (0, 1):
        out = np.full(f.limbs, 0x77, dtype=np.uint64)
        for bad in (0, r, r + 1, (1 << (64 * f.limbs)) - 1):
            assert lib.amdmsm_fr_inverse(curve, ptr(_rec(bad, f.limbs)), plain, ptr(out)) == BAD_ARG
            assert (out == 0x77).all()
        assert lib.amdmsm_fr_inverse(curve, None, plain, ptr(out)) == BAD_ARG
        assert lib.amdmsm_fr_inverse(curve, ptr(_rec(1, f.limbs)), plain, None) == BAD_ARG
        assert lib.amdmsm_fr_inverse(9, ptr(_rec(1, f.limbs)), plain, ptr(out)) == UNSUPPORTED
    with pytest.raises(ValueError):
        libff_amd.fr_inverse(curve, 0)
    with pytest.raises(ValueError):
        libff_amd.fr_inverse(curve, r)


@pytest.mark.parametrize("curve", CURVES)
def test_plan_counts_what_the_model_counts(lib, curve):
    from libff_amd import plan_fr_scan

    f = model.field(curve)
    rec = f.limbs * 8
    base = plan_fr_scan(curve, 0)
    lo, hi = base["tile_min"], base["tile_max"]
    assert lo <= hi and 1 << lo <= 1 << 8, "the smallest tile is at most 2^8 records"
    assert plan_fr_scan(curve, 0, tile_log2=lo)["spine_step"] * (1 << lo) <= 1 << 17, "the second spine step is within reach of a test"
    assert lo <= (base["tile"].bit_length() - 1) <= hi
    for tl in range(lo, hi + 1):
        T, S = 1 << tl, plan_fr_scan(curve, 0, tile_log2=tl)["spine_step"]
        for n in (0, 1, 2, T - 1, T, T + 1, 3 * T + 5, 64 * T, 64 * T + 1, 129 * T, S * T - 1, S * T, S * T + 1, 1 << 20, 1 << 28):
            for a, b, inv in ((True, False, False), (True, True, False), (False, True, False), (False, False, True)):
                got = plan_fr_scan(curve, n, a=a, b=b, invert=inv, tile_log2=tl)
                want = model.plan(n, tl, rec, a=a, b=b, invert=inv)
                assert {k: got[k] for k in want} == want, (tl, n, a, b, inv)
                assert (got["tile_min"], got["tile_max"]) == (lo, hi)
    # the default tile is one of them, and reverse / exclusive change nothing the plan reports
    d = plan_fr_scan(curve, 5000, a=True, b=True)
    assert d == plan_fr_scan(curve, 5000, a=True, b=True, tile_log2=d["tile"].bit_length() - 1)
    assert d == plan_fr_scan(curve, 5000, a=True, b=True, reverse=True, exclusive=True)


def test_plan_refusals(lib):
    out = (ctypes.c_size_t * 8)()
    call = lambda curve, n, kind, tl, o=out: lib.amdmsm_plan_fr_scan(curve, ctypes.c_size_t(n), kind, tl, o)
    assert call(0, 100, KIND_A, 0) == OK
    lo, hi = out[3], out[4]
    assert call(6, 100, KIND_A, 0) == UNSUPPORTED and call(-1, 100, KIND_A, 0) == UNSUPPORTED
    assert call(0, 100, KIND_A, 0, None) == BAD_ARG
    assert call(0, 100, 0, 0) == BAD_ARG                      # names nothing
    assert call(0, 100, REVERSE | EXCLUSIVE, 0) == BAD_ARG
    assert call(0, 100, KIND_A | 4, 0) == BAD_ARG             # an unknown flag
    assert call(0, 100, KIND_A | 0x800, 0) == BAD_ARG
    assert call(0, 100, KIND_INVERT | KIND_A, 0) == BAD_ARG
    assert call(0, 100, KIND_INVERT | REVERSE, 0) == BAD_ARG
    assert call(0, 100, KIND_INVERT, 0) == OK
    assert call(0, 100, KIND_A, lo - 1) == BAD_ARG and call(0, 100, KIND_A, hi + 1) == BAD_ARG and call(0, 100, KIND_A, -3) == BAD_ARG
    assert call(0, 100, KIND_B, lo) == OK and call(0, 100, KIND_A | KIND_B | REVERSE | EXCLUSIVE, hi) == OK
    assert call(0, (1 << 28) + 1, KIND_A, 0) == TOO_LARGE and call(0, 1 << 28, KIND_A, 0) == OK


class _Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


@pytest.mark.parametrize("curve", [0, 4, 2])
def test_refusals_come_before_the_context(lib, curve):
    """every argument rule of the four entries, with no context at all: the code alone (a call that passed them would
    answer BAD_ARG for the missing context too, so each refusal is paired with the code its rule gives, and the rules
    that answer another code -- UNSUPPORTED, TOO_LARGE -- show that the context was not what refused)"""
    f = model.field(curve)
    limbs = f.limbs
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    vec, out, one = np.ones((4, limbs), dtype=np.uint64), np.full((4, limbs), 0x5a, dtype=np.uint64), _rec(1, limbs)
    tot = np.full(limbs, 0x5a, dtype=np.uint64)
    o = _Opts(ctypes.sizeof(_Opts), 0, 0, 1, 1, 0, None)
    sz = ctypes.c_size_t
    for entry in (lib.amdmsm_fr_scan, lib.amdmsm_fr_scan_device):
        scan = lambda c, n, a, ac, b, init, flags, tl, opts=o: entry(None, c, sz(n), ptr(a), ptr(ac), ptr(b), ptr(init), flags, tl,
                                                                      ctypes.byref(opts), ptr(out), ptr(tot))
        assert scan(7, 4, vec, None, None, None, 0, 0) == UNSUPPORTED
        assert scan(curve, (1 << 28) + 1, vec, None, None, None, 0, 0) == TOO_LARGE
        assert scan(curve, 4, vec, None, None, None, 0, 0) == BAD_ARG   # the missing context, after every rule
    for entry in (lib.amdmsm_fr_batch_invert_device,):
        assert entry(None, 7, sz(4), ptr(vec), 0, ctypes.byref(o), ptr(out), None) == UNSUPPORTED
        assert entry(None, curve, sz((1 << 28) + 1), ptr(vec), 0, ctypes.byref(o), ptr(out), None) == TOO_LARGE
        assert entry(None, curve, sz(4), ptr(vec), 0, ctypes.byref(o), ptr(out), None) == BAD_ARG
    assert lib.amdmsm_fr_batch_invert(None, 7, sz(4), ptr(vec), ctypes.byref(o), ptr(out), None) == UNSUPPORTED
    assert lib.amdmsm_fr_batch_invert(None, curve, sz((1 << 28) + 1), ptr(vec), ctypes.byref(o), ptr(out), None) == TOO_LARGE
    assert (out == 0x5a).all() and (tot == 0x5a).all() and one[0] == 1


def test_layout_code_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fr_scan_layout_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "libff_amd", "csrc"), os.path.join(ROOT, "tools", "fr_scan_layout_check.cpp"), "-o", exe]
    plain = [c for c in cmd if not c.startswith("-f")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        # the same program without the sanitizers must build: then it is their runtime that is missing
        assert subprocess.run(plain, capture_output=True, text=True).returncode == 0, built.stderr[-2000:]
        pytest.skip("the host compiler has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1][:200])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().endswith("ok")
