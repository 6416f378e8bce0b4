"""The sparse matrix over Fr (amdmsm_plan_fr_matrix, amdmsm_fr_matrix_load / _apply / _apply_device / _free) as far as
a host without a GPU can see it: the symbols are exported and declared, the Python layer has the methods, the plan entry
counts classes as the integer model does and refuses what the load refuses, the accumulators' bounds hold for the six
moduli in Python integers, the model agrees with itself, and the host code that rearranges a matrix runs clean under
the host compiler's sanitizers (tools/fr_matrix_layout_check.cpp, a program of its own)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import fr_matrix_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_plan_fr_matrix", "amdmsm_fr_matrix_load", "amdmsm_fr_matrix_apply", "amdmsm_fr_matrix_apply_device",
         "amdmsm_fr_matrix_free")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5
CURVES = sorted(model.CURVES)
PLAN_WORDS = 16


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
    assert f"#define AMDMSM_FR_MATRIX_PLAN_WORDS {PLAN_WORDS}" in header and e.FR_MATRIX_PLAN_WORDS == PLAN_WORDS


def test_python_layer_has_the_methods():
    import libff_amd

    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(libff_amd.plan_fr_matrix) == ["curve", "offsets", "cols", "coeffs", "n_cols", "plain"]
    assert sig(libff_amd.Engine.fr_matrix_load) == ["self", "curve", "offsets", "cols", "coeffs", "n_cols", "plain"]
    assert sig(libff_amd.Engine.fr_matrix_apply) == ["self", "mat", "x", "n_out", "plain"]
    assert sig(libff_amd.Engine.fr_matrix_apply_device) == ["self", "mat", "d_x", "n_x", "d_out", "n_out", "plain", "stream"]
    assert "plan_fr_matrix" in libff_amd.__all__
    for name in ("free", "__enter__", "__exit__"):
        assert callable(getattr(libff_amd.FrMatrix, name))


def test_the_model_agrees_with_itself():
    for curve in CURVES:
        f = model.field(curve)
        m = model.random_matrix(f.r, [0, 1, 2, 3, 7, 40, 0, 5], 9, seed=curve, nonzero=False)
        x = model.random_x(f.r, 11, seed=100 + curve)
        assert model.apply(m, x, f.r, 10) == model.apply_dense(m, x, f.r, 10)
        for plain in (False, True):
            assert f.ints(f.records(x, plain), plain) == x


def small_matrix(f):
    """a fixed matrix with every coefficient class, repeated and unsorted columns, an empty row"""
    r = f.r
    rows = [[(2, 1), (0, r - 1), (2, 1)], [], [(4, 7), (1, 0), (3, r - 2)], [(0, 1)], [(4, 0), (4, 0)],
            [(c % 5, (1, r - 1, 2, 0, 12345)[c % 5]) for c in range(40)]]
    return model.Csr(rows, 5)


@pytest.mark.parametrize("curve", CURVES)
def test_plan_counts_what_the_model_counts(lib, curve):
    from libff_amd import plan_fr_matrix

    f = model.field(curve)
    m = small_matrix(f)
    for plain in (False, True):
        p = plan_fr_matrix(curve, *m.arrays(f, plain), m.n_cols, plain=plain)
        assert p["nnz"] == m.nnz
        assert {k: p[k] for k in ("general", "plus_one", "minus_one", "zero")} == model.class_counts(m, f.r)
        lens = model.row_lengths(m)
        assert p["longest_row"] == max(lens)
        t1, t2 = p["wave_row"], p["split_row"]
        assert 1 <= t1 <= t2
        assert p["rows_lane"] == sum(n < t1 for n in lens)
        assert p["rows_wave"] == sum(t1 <= n <= t2 for n in lens)
        assert p["rows_split"] == sum(n > t2 for n in lens)
        assert p["launches"] == (2 if p["rows_split"] else 1)
        assert p["device_bytes"] > 0
        assert p["chunk"] == model.chunk_rule(f.r, f.words)
    # no rows, and rows without entries
    empty = plan_fr_matrix(curve, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros((0, f.limbs), dtype=np.uint64), 0)
    assert empty["nnz"] == 0 and empty["rows_lane"] == 0 and empty["launches"] == 1
    rows3 = plan_fr_matrix(curve, np.zeros(4, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros((0, f.limbs), dtype=np.uint64), 7)
    assert rows3["rows_lane"] == 3 and rows3["longest_row"] == 0


def raw_plan(lib, curve, n_rows, n_cols, offsets, cols, coeffs, plain, out=True):
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    words = (ctypes.c_size_t * PLAN_WORDS)()
    return lib.amdmsm_plan_fr_matrix(curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(offsets), ptr(cols), ptr(coeffs),
                                     int(plain), words if out else None)


@pytest.mark.parametrize("curve", CURVES)
def test_plan_refuses_what_the_load_refuses(lib, curve):
    f = model.field(curve)
    m = small_matrix(f)
    off, cols, co = m.arrays(f, True)
    assert raw_plan(lib, curve, m.n_rows, m.n_cols, off, cols, co, True) == OK
    assert raw_plan(lib, 17, m.n_rows, m.n_cols, off, cols, co, True) == UNSUPPORTED
    assert raw_plan(lib, curve, m.n_rows, m.n_cols, off, cols, co, True, out=False) == BAD_ARG
    bad = off.copy()
    bad[0] = 1
    assert raw_plan(lib, curve, m.n_rows, m.n_cols, bad, cols, co, True) == BAD_ARG
    bad = off.copy()
    bad[2] = bad[1] - 1   # a decreasing offset
    assert raw_plan(lib, curve, m.n_rows, m.n_cols, bad, cols, co, True) == BAD_ARG
    assert raw_plan(lib, curve, m.n_rows, m.n_cols - 1, off, cols, co, True) == BAD_ARG   # column 4 >= n_cols = 4
    for plain in (False, True):   # a coefficient that is r itself, and one above it, in either form
        for v in (f.r, f.r + 5):
            big = m.arrays(f, plain)[2].copy()
            big[3] = np.frombuffer(v.to_bytes(8 * f.limbs, "little"), dtype="<u8")
            assert raw_plan(lib, curve, m.n_rows, m.n_cols, off, cols, big, plain) == BAD_ARG
    for missing in range(3):   # a null array with work to do
        arrs = [off, cols, co]
        arrs[missing] = None
        assert raw_plan(lib, curve, m.n_rows, m.n_cols, *arrs, True) == BAD_ARG
    # nothing to do: no array is looked at
    assert raw_plan(lib, curve, 0, 0, None, None, None, True) == OK
    assert raw_plan(lib, curve, 2, 3, np.zeros(3, dtype=np.uint64), None, None, True) == OK


def test_size_limits(lib):
    f = model.field(0)
    off, cols, co = model.Csr([[(0, 1)]], 1).arrays(f, True)
    assert raw_plan(lib, 0, (1 << 28) + 1, 1, off, cols, co, True) == TOO_LARGE   # refused before the offsets are read
    assert raw_plan(lib, 0, 1, (1 << 28) + 1, off, cols, co, True) == TOO_LARGE
    assert raw_plan(lib, 0, 1, 1 << 28, off, cols, co, True) == OK
    huge = np.array([0, (1 << 31) + 1], dtype=np.uint64)
    assert raw_plan(lib, 0, 1, 1, huge, cols, co, True) == TOO_LARGE               # nnz, before an entry is read


@pytest.mark.parametrize("curve", CURVES)
def test_accumulator_bounds(lib, curve):
    """fr_matrix.inc: T general products are summed in 2N words and reduced once into N words; the +-1 records and the
    reduced chains are summed in N + 1 words and made canonical by two Montgomery products.  Worst operands r - 1."""
    from libff_amd import plan_fr_matrix

    f = model.field(curve)
    r, N, R = f.r, f.words, f.R
    T = plan_fr_matrix(curve, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros((0, f.limbs), dtype=np.uint64), 0)["chunk"]
    assert T == model.chunk_rule(r, N) and T >= 1
    # the rule by the top word admits T and, unless the cap of 1024 chose T, not T + 1
    assert model.rule_holds(r, N, T)
    assert T == 1024 or not model.rule_holds(r, N, T + 1)
    # exact integers: the chain of T worst products fits, with the reduction's m r on top, and its reduced value fits N
    # words for every m the reduction can choose
    worst = T * (r - 1) * (r - 1)
    assert model.chain_fits(r, N, T)
    assert worst + (R - 1) * r < R * R and (worst + (R - 1) * r) // R < R
    # and the rule is no wider than the width: where it stops below the cap, a chain not much longer would not fit
    if T < 1024:
        assert not model.chain_fits(r, N, (T + 1) * 2)
    # the reduced chain of a real worst case, as the reduction computes it
    m = (-worst * pow(r, -1, R)) % R
    red = (worst + m * r) // R
    assert (worst + m * r) % R == 0 and red < R and red % r == worst * pow(R, -1, r) % r
    # the row accumulator: at most 2^20 entries per wave job (the largest split length), each adding a value below R,
    # and as many chains; 64 lanes are then added up: the carry word holds the count
    assert (2 * (1 << 20) + 1) * 64 < 1 << 32
    # r - x for a subtraction is below R for every x <= r, and adds -x
    for x in (0, 1, r - 1):
        assert 0 <= r - x < R and (r - x) % r == -x % r
    # canonical form of lo + hi R^(1): lo (R mod r) / R and hi (R^2 mod r) / R are Montgomery products of an operand below R
    # by one below r: below 2 r before the conditional subtraction, and 2 r fits N words
    lo, hi = R - 1, (1 << 32) - 1
    for a, b in ((lo, R % r), (hi, R * R % r)):
        mm = (-a * b * pow(r, -1, R)) % R
        assert (a * b + mm * r) // R < 2 * r < R
    assert (lo * (R % r) * pow(R, -1, r) + hi * (R * R % r) * pow(R, -1, r)) % r == (lo + hi * R) % r


def test_layout_code_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fr_matrix_layout_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "libff_amd", "csrc"), os.path.join(ROOT, "tools", "fr_matrix_layout_check.cpp"), "-o", exe]
    plain = [c for c in cmd if not c.startswith("-f")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        # the same program without the sanitizers must build: then it is their runtime that is missing
        assert subprocess.run(plain, capture_output=True, text=True).returncode == 0, built.stderr[-2000:]
        pytest.skip("the host compiler has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1][:200])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().endswith("ok")
