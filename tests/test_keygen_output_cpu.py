"""The key-generator output path (amdmsm_batch_exp_device, amdmsm_disk_encode_device, amdmsm_write_points_stream / _file,
amdmsm_plan_write_points) as far as a host without a GPU can see it: the symbols are exported, declared and bound, the
Engine has its methods, the refusals that come before the context is looked at, and the writers' chunk plan."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdmsm_batch_exp_device", "amdmsm_disk_encode_device", "amdmsm_write_points_stream", "amdmsm_write_points_file",
         "amdmsm_plan_write_points")
METHODS = ("batch_exp_device", "disk_encode_device", "disk_encode", "write_points_file", "write_points_stream")
BAD_ARG, UNSUPPORTED = -2, -3
ALL_GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1)]
A_NONZERO = [(4, 1), (4, 2), (5, 1)]
SIZES = (0, 1, 63, 64, 65, 128, 193)
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return libff_amd.load_library()


def test_the_symbols_are_exported_declared_and_bound(lib):
    import libff_amd.engine as e

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "amdmsm.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in e.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"typedef\s+size_t\s*\(\*amdmsm_write_fn\)\(void \*write_ctx, const void \*src, size_t bytes\)", header)
    src = inspect.getsource(e.Engine)
    for name in NAMES[:4]:
        assert "self.lib.%s(" % name in src, name
    assert "amdmsm_plan_write_points(" in inspect.getsource(e.plan_write_points)


def test_the_engine_has_the_five_methods():
    import libff_amd
    from libff_amd import OUT_LIBFF, multi_exp_base_form_normal

    for m in METHODS:
        assert callable(getattr(libff_amd.Engine, m, None)), m
    par = lambda m: inspect.signature(getattr(libff_amd.Engine, m)).parameters
    p = par("batch_exp_device")
    assert list(p)[1:] == ["curve", "group", "scalar_size", "window", "g", "d_scalars", "n", "d_out_xyz", "coeff",
                           "scalars_plain", "out_form", "stream"]
    assert p["coeff"].default is None and p["scalars_plain"].default is False and p["out_form"].default == OUT_LIBFF
    p = par("disk_encode_device")
    assert list(p)[1:] == ["curve", "group", "d_points_affine", "n", "d_records", "compressed", "stream"]
    p = par("disk_encode")
    assert list(p)[1:] == ["curve", "group", "points_xyz", "compressed", "base_form"]
    assert p["compressed"].default is False and p["base_form"].default == multi_exp_base_form_normal
    p = par("write_points_file")
    assert list(p)[1:] == ["curve", "group", "d_points_affine", "n", "path", "offset_bytes", "compressed", "chunk_points"]
    assert p["offset_bytes"].default == 0 and p["chunk_points"].default == 0
    p = par("write_points_stream")
    assert list(p)[1:] == ["curve", "group", "d_points_affine", "n", "writer", "compressed", "chunk_points"]


def _calls(lib, curve, group, compressed=0, scalar_size=64, window=5):
    """every new entry that takes a context, with a null one"""
    return {
        "batch_exp_device": lambda: lib.amdmsm_batch_exp_device(None, curve, group, SZ(scalar_size), SZ(window), None, None, SZ(0),
                                                                None, None, None),
        "disk_encode_device": lambda: lib.amdmsm_disk_encode_device(None, curve, group, None, SZ(0), compressed, None, None),
        "write_points_stream": lambda: lib.amdmsm_write_points_stream(None, curve, group, None, SZ(0), compressed, None, None, SZ(0)),
        "write_points_file": lambda: lib.amdmsm_write_points_file(None, curve, group, None, SZ(0), compressed, None, SZ(0), SZ(0)),
    }


def test_mnt6_g2_is_unsupported_before_the_context_is_looked_at(lib):
    for compressed in (0, 1):
        for what, call in _calls(lib, 5, 2, compressed).items():
            assert call() == UNSUPPORTED, (what, compressed)
    for what, call in _calls(lib, 7, 1).items():
        assert call() == UNSUPPORTED, what


@pytest.mark.parametrize("curve,group", ALL_GROUPS)
def test_compressed_records_of_the_a_nonzero_curves(lib, curve, group):
    """UNSUPPORTED for (MNT4, G1 / G2) and (MNT6, G1), again before the context; the other groups get as far as the null
    context, which is BAD_ARG"""
    want = UNSUPPORTED if (curve, group) in A_NONZERO else BAD_ARG
    calls = _calls(lib, curve, group, 1)
    for what in ("disk_encode_device", "write_points_stream", "write_points_file"):
        assert calls[what]() == want, what
    calls = _calls(lib, curve, group, 0)
    for what in ("disk_encode_device", "write_points_stream", "write_points_file"):
        assert calls[what]() == BAD_ARG, what


@pytest.mark.parametrize("curve,group", ALL_GROUPS)
def test_window_and_scalar_size(lib, curve, group):
    import libff_amd

    bits = libff_amd.sizes(curve, group)["fr_bytes"] * 8   # the largest scalar_size amdmsm_batch_exp accepts
    for scalar_size, window in ((bits, 0), (bits, 23), (0, 5), (bits + 1, 5)):
        assert _calls(lib, curve, group, 0, scalar_size, window)["batch_exp_device"]() == BAD_ARG, (scalar_size, window)
    # in range: nothing to refuse but the null context
    assert _calls(lib, curve, group, 0, bits, 22)["batch_exp_device"]() == BAD_ARG


@pytest.mark.parametrize("chunk", [64, 1, 0])
def test_the_chunk_plan_covers_every_record_once(lib, chunk):
    import libff_amd

    assert lib.amdmsm_plan_write_points(SZ(5), SZ(chunk), SZ(0), None) == BAD_ARG
    for n in SIZES:
        chunks = libff_amd.plan_write_points(n, chunk)
        size = min(chunk or 1 << 20, n) if n else 0
        assert len(chunks) == (-(-n // size) if n else 0), (n, chunk)
        at = 0
        for k, (first, count, buffer) in enumerate(chunks):
            assert first == at and 1 <= count <= size and buffer == k % 2, (n, chunk, k)
            assert count == size or k == len(chunks) - 1, (n, chunk, k)
            at += count
        assert at == n, (n, chunk)
        # past the last chunk: the count alone
        out = (SZ * 4)(7, 7, 7, 7)
        assert lib.amdmsm_plan_write_points(SZ(n), SZ(chunk), SZ(len(chunks)), out) == 0
        assert list(out) == [len(chunks), 0, 0, 0]


def test_the_default_chunk_is_the_readers(lib):
    import libff_amd

    chunks = libff_amd.plan_write_points((1 << 21) + 3, 0)
    assert chunks == [(0, 1 << 20, 0), (1 << 20, 1 << 20, 1), (1 << 21, 3, 0)]


def test_the_chunk_plan_under_the_host_sanitizers(tmp_path):
    """tools/write_plan_check.cpp, a program of its own: the plan walked as write_impl walks it, every buffer a heap block
    of its exact size"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "write_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "libff_amd", "csrc"), os.path.join(ROOT, "tools", "write_plan_check.cpp"), "-o", exe]
    plain = [c for c in cmd if not c.startswith("-f")]
    # compiling under the sanitizers needs no runtime: an error there is the program's, never a reason to skip
    obj = str(tmp_path / "write_plan_check.o")
    compiled = subprocess.run(cmd[:-2] + ["-c", "-o", obj], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr[-2000:]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        # the link alone fails, and the same program without the sanitizers builds: it is their runtime that is missing
        assert subprocess.run(plain, capture_output=True, text=True).returncode == 0, built.stderr[-2000:]
        pytest.skip("the host compiler has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1][:200])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().endswith("ok")
