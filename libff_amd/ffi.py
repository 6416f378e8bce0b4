"""The FFI-convention entry points (include/libff_amd_ffi.h) over byte buffers.

Everything crosses in libff's wire format (ffi_serialization.tcc): big-endian plain integers, affine X || Y, Fq2
coordinates c1 then c0, zero = (0, 1).  ``bases`` / ``scalars`` are ``bytes``-like objects or uint8 arrays.  A function
returns ``None`` exactly where its C call returns ``false`` (wrong size, element out of range, off the curve or outside
the safe subgroup, unknown handle, range past the vector); a curve / group pair the library has no symbol for raises.

    multiexp(curve, group, bases, scalars)            <curve>_g{1,2}_multiexp, validates every base on every call
    h = load_bases(curve, group, bases)               validates once, keeps the decoded vector in HBM
    multiexp_loaded(h, scalars, first_point=0)        scalars against points first_point ... of the loaded vector
    free_bases(h)
    element_sizes(curve, group)                       {"fr_bytes", "element_bytes"} of the wire format (no GPU needed)

Helpers beside those five: GROUPS (the eleven (curve, group) pairs), symbol_name(curve, group) (the C name of the
one-shot entry) and last_timings() (amdmsm_ffi_last_timings: three device times in ms of the last call).

The None rule holds for free_bases too: True when the vector was released, None (not False) for a handle that is
unknown or already freed, so that every function of this module signals a refused call the same way.  load_bases
returns a LoadedBases, an int that also carries (curve, group, n); multiexp_loaded needs that object, because the size
of its output follows from the group, and raises TypeError for a bare int.  free_bases needs only the number.
"""
import ctypes

import numpy as np

from . import engine as _e

_PREFIX = {_e.ALT_BN128: "alt_bn128", _e.BLS12_377: "bls12_377", _e.BW6_761: "bw6_761", _e.BLS12_381: "bls12_381",
           _e.MNT4: "mnt4", _e.MNT6: "mnt6"}
# every (curve, group) pair with an FFI symbol: all of the engine's groups (MNT6 G2 is unsupported everywhere)
GROUPS = [(c, g) for c in _PREFIX for g in (_e.G1, _e.G2) if (c, g) != (_e.MNT6, _e.G2)]


def _curve_id(curve):
    if isinstance(curve, str):
        for k, v in _PREFIX.items():
            if v == curve:
                return k
        raise _e.AmdMsmError(f"unknown curve {curve!r}")
    return int(curve)


def symbol_name(curve, group):
    curve = _curve_id(curve)
    if (curve, group) not in GROUPS:
        raise _e.AmdMsmError(f"no FFI entry for curve {curve} group {group}")
    return f"{_PREFIX[curve]}_g{group}_multiexp"


def element_sizes(curve, group):
    """Wire sizes in bytes: an Fr element and a group element (affine X || Y)."""
    curve = _curve_id(curve)
    symbol_name(curve, group)
    s = _e.sizes(curve, group)
    return {"fr_bytes": int(s["fr_bytes"]), "element_bytes": int(s["affine_bytes"])}


def _buf(x):
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.asarray(x)
    if a.dtype != np.uint8:
        raise TypeError("byte buffers are bytes-like or uint8 arrays")
    return np.ascontiguousarray(a).reshape(-1)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else None)


def multiexp(curve, group, bases, scalars):
    """sum scalars[i] * bases[i] as the encoded affine element (bytes), or None where the call returns false."""
    curve = _curve_id(curve)
    fn = getattr(_e.load_library(), symbol_name(curve, group))
    fn.restype = ctypes.c_bool
    b, s = _buf(bases), _buf(scalars)
    out = np.zeros(element_sizes(curve, group)["element_bytes"], dtype=np.uint8)
    ok = fn(_ptr(b), ctypes.c_size_t(b.size), _ptr(s), ctypes.c_size_t(s.size), _ptr(out), ctypes.c_size_t(out.size))
    return out.tobytes() if ok else None


class LoadedBases(int):
    """Handle of amdmsm_ffi_bases_load (an int) that remembers its group, so that the output can be sized."""

    def __new__(cls, value, curve, group, n):
        h = super().__new__(cls, value)
        h.curve, h.group, h.n = curve, group, n
        return h


def load_bases(curve, group, bases):
    """Validate `bases` once and keep the decoded vector on the device: a handle, or None where any element fails."""
    curve = _curve_id(curve)
    symbol_name(curve, group)
    lib = _e.load_library()
    lib.amdmsm_ffi_bases_load.restype = ctypes.c_bool
    b = _buf(bases)
    h = ctypes.c_uint64(0)
    ok = lib.amdmsm_ffi_bases_load(ctypes.c_int(curve), ctypes.c_int(group), _ptr(b), ctypes.c_size_t(b.size),
                                   ctypes.byref(h))
    if not ok:
        return None
    return LoadedBases(h.value, curve, group, b.size // element_sizes(curve, group)["element_bytes"])


def multiexp_loaded(handle, scalars, first_point=0):
    """n = len(scalars) / Fr bytes scalars against points first_point ... first_point + n - 1 of a loaded vector."""
    if not isinstance(handle, LoadedBases):
        raise TypeError("handle: what load_bases returned")
    lib = _e.load_library()
    lib.amdmsm_ffi_multiexp_loaded.restype = ctypes.c_bool
    s = _buf(scalars)
    out = np.zeros(element_sizes(handle.curve, handle.group)["element_bytes"], dtype=np.uint8)
    ok = lib.amdmsm_ffi_multiexp_loaded(ctypes.c_uint64(int(handle)), ctypes.c_size_t(first_point), _ptr(s),
                                        ctypes.c_size_t(s.size), _ptr(out), ctypes.c_size_t(out.size))
    return out.tobytes() if ok else None


def free_bases(handle):
    """Release a loaded vector: True, or None for a handle that is unknown or already freed."""
    lib = _e.load_library()
    lib.amdmsm_ffi_bases_free.restype = ctypes.c_bool
    return True if lib.amdmsm_ffi_bases_free(ctypes.c_uint64(int(handle))) else None


def last_timings():
    """Device milliseconds of the last call (amdmsm_ffi_last_timings), or None before the first one."""
    lib = _e.load_library()
    lib.amdmsm_ffi_last_timings.restype = ctypes.c_bool
    ms = (ctypes.c_float * 3)()
    return [float(x) for x in ms] if lib.amdmsm_ffi_last_timings(ms) else None
