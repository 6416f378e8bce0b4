"""What the GPU tests of the Fr-vector entries (test_gpu_fr_*.py) share: device buffers freed together, the HIP runtime
for a stream of the test's own, an environment switch held for a block, the return codes, and Horner's rule."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE = 0, -2, -3, -5   # include/amdmsm.h AMDMSM_OK / AMDMSM_ERR_*
SENTINEL = 0x5a5a5a5a5a5a5a5a
# 8, 10 and 12 words, and bls12_381 for its chain of two products
FOUR = [pytest.param(0, id="alt_bn128"), pytest.param(4, id="mnt4"), pytest.param(2, id="bw6_761"), pytest.param(3, id="bls12_381")]


class Dev:
    """device buffers of a test, freed together"""

    def __init__(self, engine):
        self.e, self.ptrs = engine, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.e.free(p)

    def buf(self, nbytes):
        p = self.e.malloc(max(nbytes, 64))
        self.ptrs.append(p)
        return p

    def up(self, arr):
        p = self.buf(arr.nbytes)
        if arr.nbytes:
            self.e.h2d(p, arr)
        return p

    def down(self, p, shape):
        out = np.zeros(shape, dtype=np.uint64)
        self.e.synchronize()
        if out.nbytes:
            self.e.d2h(out, p)
        return out


def at(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def hip_runtime():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise AssertionError("libamdhip64.so not found")


@contextlib.contextmanager
def env_path(name, on):
    """the environment of a block: the switch ``name`` set to 1 or absent, and as it was afterwards"""
    old = os.environ.pop(name, None)
    if on:
        os.environ[name] = "1"
    try:
        yield
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


def poly_eval(coeffs, t, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * t + c) % r
    return acc
