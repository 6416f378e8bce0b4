"""ctypes binding of libamdmsm.so -- the host-side mirror of libff's multi_exp interface.

The names follow the reference (libff/algebra/scalar_multiplication/multiexp.hpp:21-141):
``multi_exp``, ``multi_exp_filter_one_zero``, ``batch_to_special``,
``bdlo12_signed_optimal_c``, the ``multi_exp_method_*`` / ``multi_exp_base_form_*`` enums.
Everything is computed by the HIP engine; there is NO CPU fallback here -- a missing
``libamdmsm.so`` or a missing GPU raises immediately.

Array conventions (numpy ``uint64``, libff's in-memory layout, see include/amdmsm.h):
  scalars  (n, fr_limbs)      Montgomery residues (as ``std::vector<Fr>`` holds them)
  bases    (n, 3*coord_limbs) (X, Y, Z) records
  result   (3*coord_limbs,)   (X, Y, Z); ``out_form`` selects the representative
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# AMDMSM_LIBRARY: another build of the same ABI (A/B runs of experimental builds, tools/)
SO_PATH = os.environ.get("AMDMSM_LIBRARY") or os.path.join(HERE, "libamdmsm.so")

# curve / group ids (include/amdmsm.h)
ALT_BN128, BLS12_377, BW6_761, BLS12_381, MNT4, MNT6 = 0, 1, 2, 3, 4, 5   # MNT4 / MNT6: G1 only
G1, G2 = 1, 2
CURVE_NAMES = {ALT_BN128: "alt_bn128", BLS12_377: "bls12_377", BW6_761: "bw6_761", BLS12_381: "bls12_381",
               MNT4: "mnt4", MNT6: "mnt6"}

# libff::multi_exp_method, multiexp.hpp:21-43
multi_exp_method_naive = 0
multi_exp_method_naive_plain = 1
multi_exp_method_bos_coster = 2
multi_exp_method_BDLO12 = 3
multi_exp_method_BDLO12_signed = 4
# libff::multi_exp_base_form, multiexp.hpp:45-51
multi_exp_base_form_normal = 0
multi_exp_base_form_special = 1

ABI_VERSION = 3   # AMDMSM_ABI_VERSION of include/amdmsm.h this file mirrors (amdmsm_opts layout)
OUT_JACOBIAN, OUT_LIBFF, OUT_AFFINE = 0, 1, 2
PH_COUNT, PH_SCATTER, PH_ACCUM, PH_REDUCE, PH_FINAL, PH_TOTAL = range(6)
MAX_PHASES = 8

EXPORTED_SYMBOLS = [
    "amdmsm_abi_version", "amdmsm_device_count", "amdmsm_ctx_create", "amdmsm_ctx_destroy", "amdmsm_strerror",
    "amdmsm_last_error", "amdmsm_sizes", "amdmsm_plan", "amdmsm_plan_ex", "amdmsm_plan_sort", "amdmsm_plan_sort_digit_grid", "amdmsm_plan_top_window", "amdmsm_endomorphism_info",
    "amdmsm_endomorphism_digits_device", "amdmsm_pippenger_optimal_c",
    "amdmsm_bdlo12_signed_optimal_c", "amdmsm_multi_exp", "amdmsm_multi_exp_batch", "amdmsm_multi_exp_batch_items",
    "amdmsm_msm_device_batch_items", "amdmsm_multi_exp_filter_one_zero",
    "amdmsm_multi_exp_multi", "amdmsm_multi_exp_filter_one_zero_multi", "amdmsm_msm_device_multi", "amdmsm_register_bases", "amdmsm_unregister_bases",
    "amdmsm_invalidate_bases",
    "amdmsm_batch_to_special", "amdmsm_batch_exp", "amdmsm_get_batch_exp_timings", "amdmsm_multi_exp_stream", "amdmsm_multi_exp_stream_file",
    "amdmsm_multi_exp_stream_compressed", "amdmsm_multi_exp_stream_compressed_file", "amdmsm_disk_decode_device",
    "amdmsm_precompute_num_digits", "amdmsm_multi_exp_stream_with_precompute",
    "amdmsm_multi_exp_stream_with_precompute_file", "amdmsm_precompute_bases_device",
    "amdmsm_msm_precomputed_device", "amdmsm_import_bases_device", "amdmsm_export_affine_device",
    "amdmsm_msm_device", "amdmsm_msm_device_batch", "amdmsm_sum_points_device", "amdmsm_gen_bases_seq_device",
    "amdmsm_set_timing", "amdmsm_get_timings", "amdmsm_last_timing_ticket", "amdmsm_get_timings_by_ticket",
    "amdmsm_set_pipeline_depth", "amdmsm_last_slot",
    "amdmsm_get_slot_timings", "amdmsm_field_op_device", "amdmsm_group_op_device",
    "amdmsm_field_probe_device", "amdmsm_xyzz_probe_device", "amdmsm_rr_probe_device", "amdmsm_xyzz_rr_probe_device",
    "amdmsm_digits_device", "amdmsm_mul_bench_device", "amdmsm_madd_bench_device", "amdmsm_malloc", "amdmsm_free",
    "amdmsm_memcpy_h2d", "amdmsm_memcpy_d2h", "amdmsm_synchronize",
    "amdmsm_plan_short", "amdmsm_scalar_bits_device", "amdmsm_multi_exp_short", "amdmsm_msm_device_short",
    "amdmsm_scalar_mul_vec", "amdmsm_scalar_mul_vec_device",
    "amdmsm_multi_exp_segments", "amdmsm_msm_device_segments", "amdmsm_set_segments_chunk_terms",
    "amdmsm_fold_vec", "amdmsm_fold_vec_device", "amdmsm_plan_fold",
    "amdmsm_group_fft", "amdmsm_group_fft_device", "amdmsm_plan_group_fft", "amdmsm_fr_modulus",
    "amdmsm_fr_fft", "amdmsm_fr_fft_device", "amdmsm_plan_fr_fft", "amdmsm_fr_root_of_unity", "amdmsm_fr_powers_device",
    "amdmsm_fr_muladd_device",
    "amdmsm_plan_fr_matrix", "amdmsm_fr_matrix_load", "amdmsm_fr_matrix_apply", "amdmsm_fr_matrix_apply_device",
    "amdmsm_fr_matrix_free",
    "amdmsm_fr_scan", "amdmsm_fr_scan_device", "amdmsm_fr_batch_invert", "amdmsm_fr_batch_invert_device", "amdmsm_plan_fr_scan",
    "amdmsm_fr_inverse",
    "amdmsm_fr_domain", "amdmsm_fr_domain_element", "amdmsm_fr_domain_vanishing", "amdmsm_fr_domain_z_terms",
    "amdmsm_fr_multiplicative_generator", "amdmsm_fr_domain_fft", "amdmsm_fr_domain_fft_device",
    "amdmsm_fr_domain_divide_by_z", "amdmsm_fr_domain_divide_by_z_device",
    "amdmsm_fr_domain_lagrange", "amdmsm_fr_domain_lagrange_device",
    "amdmsm_fr_matrix_load_transposed", "amdmsm_plan_fr_matrix_transposed", "amdmsm_fr_lincomb_device",
    "amdmsm_batch_exp_device", "amdmsm_disk_encode_device", "amdmsm_write_points_stream", "amdmsm_write_points_file",
    "amdmsm_plan_write_points",
    "amdmsm_fr_fft_batch", "amdmsm_fr_fft_batch_device", "amdmsm_plan_fr_fft_batch", "amdmsm_fr_domain_fft_batch_device",
    "amdmsm_fr_qap_witness_map", "amdmsm_fr_qap_witness_map_device", "amdmsm_plan_fr_qap_witness_map",
    "amdmsm_group_matrix_apply", "amdmsm_group_matrix_apply_device", "amdmsm_plan_group_matrix",
]
SEG_SHARED_BASES = 1            # include/amdmsm.h AMDMSM_SEG_SHARED_BASES
SEG_LONG_NEVER = 2 ** 64 - 1    # long_from = SIZE_MAX: no segment takes the single-MSM route
# amdmsm_scalar_desc.kind: Fr records, or the width in bytes of packed little-endian unsigned integers
SCALAR_FR, SCALAR_U8, SCALAR_U16, SCALAR_U32, SCALAR_U64 = 0, 1, 2, 4, 8


class AmdMsmError(RuntimeError):
    pass


class _Opts(ctypes.Structure):
    # include/amdmsm.h amdmsm_opts, AMDMSM_ABI_VERSION 3 (struct_size first)
    _fields_ = [("struct_size", ctypes.c_uint32), ("window_bits", ctypes.c_int), ("segment_len", ctypes.c_int),
                ("out_form", ctypes.c_int), ("scalars_plain", ctypes.c_int), ("endomorphism", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


class BatchItemStruct(ctypes.Structure):
    # include/amdmsm.h amdmsm_batch_item
    _fields_ = [("struct_size", ctypes.c_uint32), ("bases", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("scalars", ctypes.c_void_p), ("shared_offset", ctypes.c_size_t), ("index", ctypes.c_void_p),
                ("out_xyz", ctypes.c_void_p)]


class ScalarDesc(ctypes.Structure):
    # include/amdmsm.h amdmsm_scalar_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_int), ("bits", ctypes.c_int)]


def scalar_desc(kind, bits=0):
    return ScalarDesc(ctypes.sizeof(ScalarDesc), int(kind), int(bits))


_INT_KINDS = {"uint8": SCALAR_U8, "uint16": SCALAR_U16, "uint32": SCALAR_U32, "uint64": SCALAR_U64}


class BatchItem:
    """One MSM of ``Engine.multi_exp_batch_items``: ``bases`` and exactly one source of scalars -- ``scalars`` (its own
    vector), ``index`` (a uint32 array into the shared vector; any order, repeats allowed) or ``offset`` (the slice
    ``shared[offset : offset + len(bases)]``; the default is the prefix)."""

    def __init__(self, bases, scalars=None, offset=0, index=None):
        self.bases, self.scalars, self.offset, self.index = bases, scalars, offset, index


_lib = None


def load_library():
    """Load libamdmsm.so (in-tree).  Raises if it has not been built: no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise AmdMsmError(
                f"{SO_PATH} is missing: build the HIP engine first (python -m libff_amd.build or "
                "__graft_entry__.build()); libff_amd has no CPU implementation")
        L = ctypes.CDLL(SO_PATH)
        if not hasattr(L, "amdmsm_abi_version") or L.amdmsm_abi_version() != ABI_VERSION:
            raise AmdMsmError(f"{SO_PATH} was built from another include/amdmsm.h (ABI version "
                              f"{L.amdmsm_abi_version() if hasattr(L, 'amdmsm_abi_version') else '< 3'}, this binding "
                              f"expects {ABI_VERSION}): rebuild with python -m libff_amd.build")
        L.amdmsm_strerror.restype = ctypes.c_char_p
        L.amdmsm_last_error.restype = ctypes.c_char_p
        L.amdmsm_last_error.argtypes = [ctypes.c_void_p]
        L.amdmsm_pippenger_optimal_c.restype = ctypes.c_size_t
        L.amdmsm_bdlo12_signed_optimal_c.restype = ctypes.c_size_t
        L.amdmsm_precompute_num_digits.restype = ctypes.c_size_t
        L.amdmsm_last_timing_ticket.restype = ctypes.c_longlong
        L.amdmsm_last_timing_ticket.argtypes = [ctypes.c_void_p]
        L.amdmsm_ctx_destroy.restype = None
        L.amdmsm_ctx_destroy.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def bdlo12_signed_optimal_c(num_entries):
    """multiexp.hpp:53-57 / multiexp.tcc:637-641"""
    return int(load_library().amdmsm_bdlo12_signed_optimal_c(ctypes.c_size_t(num_entries)))


def precompute_num_digits(curve, c):
    """(Fr::num_bits + c - 1) / c: multiples per base in a precompute file (multiexp_stream.tcc:205)."""
    lib = load_library()
    return int(lib.amdmsm_precompute_num_digits(curve, ctypes.c_size_t(c)))


def pippenger_optimal_c(num_elements):
    """multiexp.tcc:35-40"""
    return int(load_library().amdmsm_pippenger_optimal_c(ctypes.c_size_t(num_elements)))


def sizes(curve, group):
    out = (ctypes.c_size_t * 4)()
    rc = load_library().amdmsm_sizes(curve, group, out)
    if rc:
        raise AmdMsmError(f"amdmsm_sizes({curve},{group}): {rc}")
    return {"fr_bytes": out[0], "g_bytes": out[1], "affine_bytes": out[2], "fr_bits": out[3]}


def plan(curve, group, n, window_bits=0, endomorphism=0):
    c, w, used = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    b = ctypes.c_uint32(0)
    ws = ctypes.c_size_t(0)
    rc = load_library().amdmsm_plan_ex(curve, group, ctypes.c_size_t(n), window_bits, endomorphism, ctypes.byref(c),
                                       ctypes.byref(w), ctypes.byref(b), ctypes.byref(ws), ctypes.byref(used))
    if rc:
        raise AmdMsmError(f"amdmsm_plan_ex: {rc}")
    return {"c": c.value, "num_windows": w.value, "num_buckets": b.value, "workspace_bytes": ws.value,
            "endomorphism": bool(used.value)}


def plan_short(curve, group, n, scalar_bits, window_bits=0, endomorphism=0):
    """``plan`` for scalars below ``2**scalar_bits`` (``amdmsm_plan_short``; 0 = full width): the windows cover
    ``scalar_bits + 2`` bits, and the endomorphism split is kept only above its own bound."""
    c, w, used = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    b = ctypes.c_uint32(0)
    ws = ctypes.c_size_t(0)
    rc = load_library().amdmsm_plan_short(curve, group, ctypes.c_size_t(n), window_bits, endomorphism, int(scalar_bits),
                                          ctypes.byref(c), ctypes.byref(w), ctypes.byref(b), ctypes.byref(ws),
                                          ctypes.byref(used))
    if rc:
        raise AmdMsmError(f"amdmsm_plan_short: {rc}")
    return {"c": c.value, "num_windows": w.value, "num_buckets": b.value, "workspace_bytes": ws.value,
            "endomorphism": bool(used.value)}


def plan_sort(curve, group, n, window_bits=0, endomorphism=0):
    """Geometry of the bucket sort behind ``plan`` (read-only): columns per window, coarse / fine bits of the bucket
    index, the longest coarse bin the fine pass sorts in one piece and the length above which a bin is spread over
    the whole grid."""
    out = (ctypes.c_size_t * 5)()
    rc = load_library().amdmsm_plan_sort(curve, group, ctypes.c_size_t(n), window_bits, endomorphism, out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_sort: {rc}")
    return {"columns": out[0], "coarse_bits": out[1], "fine_bits": out[2], "chunk_cap": out[3], "big_thresh": out[4]}


def plan_sort_digit_grid(items, workgroups, block_min=0):
    """Grid of the sort's digit pass over ``items`` work items on a device that holds ``workgroups`` of its workgroups
    at once (read-only): workgroup g walks blocks g, g + grid, ... of ``block`` consecutive items."""
    out = (ctypes.c_size_t * 3)()
    rc = load_library().amdmsm_plan_sort_digit_grid(ctypes.c_size_t(items), int(block_min), int(workgroups), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_sort_digit_grid: {rc}")
    return {"block": out[0], "blocks": out[1], "grid": out[2]}


def plan_fold(curve, group, k, n, chunk_points=0, endomorphism=0):
    """What ``Engine.fold_vec`` runs for ``k`` vectors of ``n`` elements (``amdmsm_plan_fold``, read-only): digit rows (k,
    or 2k with the endomorphism split), windows per row, whether the split is used, elements per chunk and the workspace
    of a chunk."""
    out = (ctypes.c_size_t * 5)()
    rc = load_library().amdmsm_plan_fold(curve, group, int(k), ctypes.c_size_t(n), ctypes.c_size_t(chunk_points),
                                         int(endomorphism), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_fold: {rc}")
    return {"rows": out[0], "num_windows": out[1], "endomorphism": bool(out[2]), "chunk_points": out[3],
            "workspace_bytes": out[4]}


def plan_group_fft(curve, group, n, chunk_points=0):
    """What ``Engine.group_fft`` runs for ``n`` points (``amdmsm_plan_group_fft``, read-only): stages, the stages that run
    a ladder, scalar multiplications in total, butterflies per chunk, workspace bytes and the part of them that scales
    with the chunk."""
    out = (ctypes.c_size_t * 6)()
    rc = load_library().amdmsm_plan_group_fft(curve, group, ctypes.c_size_t(n), ctypes.c_size_t(chunk_points), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_group_fft: {rc}")
    return {"stages": out[0], "ladder_stages": out[1], "scalar_muls": out[2], "chunk_points": out[3],
            "workspace_bytes": out[4], "chunk_bytes": out[5]}


def fr_modulus(curve, group):
    """The scalar-field modulus r of the group (``amdmsm_fr_modulus``), as an int."""
    r = (ctypes.c_uint8 * sizes(curve, group)["fr_bytes"])()
    rc = load_library().amdmsm_fr_modulus(curve, group, r)
    if rc:
        raise AmdMsmError(f"amdmsm_fr_modulus: {rc}")
    return int.from_bytes(bytes(r), "little")


def fft_twiddles(curve, n, inverse=False):
    """The twiddles of ``Engine.group_fft`` for ``n`` points (a power of two): the (n / 2, fr_limbs) uint64 array of the
    plain powers w^0 .. w^(n/2 - 1) of an n-th root of unity w = g^((r - 1) / n), g the smallest of 2, 3, 5, ... for which
    w^(n/2) = r - 1 -- pass them with ``scalars_plain=True``.  ``inverse``: the powers of w^-1 instead.  ValueError where
    n does not divide the 2-part of r - 1."""
    n = int(n)
    r = fr_modulus(curve, G1)
    limbs = _fr_limbs(curve)
    if n < 1 or n & (n - 1):
        raise ValueError(f"n = {n} is not a power of two")
    if (r - 1) % n:
        raise ValueError(f"n = {n} does not divide r - 1 of {CURVE_NAMES.get(curve, curve)}: no n-th root of unity in Fr")
    w = 1
    if n > 1:
        g = 2
        while True:
            if all(g % q for q in range(2, g)):   # g prime
                w = pow(g, (r - 1) // n, r)
                if pow(w, n // 2, r) == r - 1:
                    break
            g += 1
    if inverse:
        w = pow(w, r - 2, r)
    buf, x = bytearray(), 1
    for _ in range(n // 2):
        buf += x.to_bytes(8 * limbs, "little")
        x = x * w % r
    return np.frombuffer(bytes(buf), dtype="<u8").astype(np.uint64).reshape(n // 2, limbs)


def plan_fr_fft(curve, n, tile_log2=0):
    """What ``Engine.fr_fft`` runs for ``n`` scalars (``amdmsm_plan_fr_fft``, read-only): butterfly stages per global pass,
    the smallest and largest such tile the unit supports, global passes, butterflies and workspace bytes."""
    out = (ctypes.c_size_t * 6)()
    rc = load_library().amdmsm_plan_fr_fft(curve, ctypes.c_size_t(n), int(tile_log2), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_fr_fft: {rc}")
    return {"tile_log2": out[0], "tile_min": out[1], "tile_max": out[2], "passes": out[3], "butterflies": out[4],
            "workspace_bytes": out[5]}


def plan_fr_fft_batch(curve, n, batch, tile_log2=0):
    """What ``Engine.fr_fft_batch`` runs for ``batch`` vectors of ``n`` scalars (``amdmsm_plan_fr_fft_batch``, read-only):
    the tile, the global passes, the vectors one workgroup holds, the workgroups and launches of the pass kernel, the
    butterflies, and the workspace bytes of an out-of-place and of an in-place device call."""
    out = (ctypes.c_size_t * 8)()
    rc = load_library().amdmsm_plan_fr_fft_batch(curve, ctypes.c_size_t(n), ctypes.c_size_t(batch), int(tile_log2), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_fr_fft_batch: {rc}")
    return {"tile_log2": out[0], "passes": out[1], "vectors_per_workgroup": out[2], "workgroups": out[3], "launches": out[4],
            "butterflies": out[5], "workspace_bytes": out[6], "workspace_bytes_in_place": out[7]}


def plan_fr_qap_witness_map(curve, m):
    """What ``Engine.qap_witness_map`` runs on the domain of ``m`` points (``amdmsm_plan_fr_qap_witness_map``, read-only):
    the domain's kind, m, B, S, the workspace bytes (without the applies' partial sums) and the launches of the batched
    pass kernel."""
    out = (ctypes.c_size_t * 6)()
    rc = load_library().amdmsm_plan_fr_qap_witness_map(curve, ctypes.c_size_t(m), out)
    if rc:
        raise _domain_error("amdmsm_plan_fr_qap_witness_map", rc)
    return {"kind": out[0], "m": out[1], "B": out[2], "S": out[3], "workspace_bytes": out[4], "batch_pass_launches": out[5]}


def fr_root_of_unity(curve, n):
    """libff's ``get_root_of_unity<Fr>(n)`` (``amdmsm_fr_root_of_unity``), as an int: what ``basic_radix2_domain`` of size
    ``n`` uses.  ValueError where n is no power of two or exceeds the 2-part of r - 1."""
    n = int(n)
    if n < 1 or n & (n - 1):
        raise ValueError(f"n = {n} is not a power of two")
    w = (ctypes.c_uint8 * sizes(curve, G1)["fr_bytes"])()
    rc = load_library().amdmsm_fr_root_of_unity(curve, n.bit_length() - 1, w)
    if rc:
        raise ValueError(f"n = {n}: no n-th root of unity in Fr of {CURVE_NAMES.get(curve, curve)} ({rc})")
    return int.from_bytes(bytes(w), "little")


FR_MATRIX_PLAN_WORDS = 16   # include/amdmsm.h AMDMSM_FR_MATRIX_PLAN_WORDS


def _csr_arrays(curve, offsets, cols, coeffs):
    """the CSR arrays as the C entries take them: uint64 offsets, uint32 columns, (nnz, fr_limbs) uint64 records"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    coeffs, _ = _fr_array(curve, coeffs)
    assert offsets.ndim == 1 and cols.ndim == 1 and cols.shape[0] == coeffs.shape[0], "cols and coeffs: one per entry"
    assert offsets.shape[0] == 0 or int(offsets[-1]) <= cols.shape[0], "offsets reach beyond the entries given"
    ptr = lambda a: _np_ptr(a) if a.size else None
    return offsets, cols, coeffs, max(0, offsets.shape[0] - 1), ptr


def plan_fr_matrix(curve, offsets, cols, coeffs, n_cols, plain=False):
    """What ``Engine.fr_matrix_load`` would build from a CSR matrix (``amdmsm_plan_fr_matrix``, read-only, no device):
    entries per coefficient class, rows per length class with the thresholds between them, the longest row, device
    bytes, launches of one apply and the field's chain length.  Validates exactly what the load validates and raises
    ``AmdMsmError`` with the code."""
    return _plan_fr_matrix("amdmsm_plan_fr_matrix", curve, offsets, cols, coeffs, n_cols, plain)


def plan_fr_matrix_transposed(curve, offsets, cols, coeffs, n_cols, plain=False):
    """What ``Engine.fr_matrix_load_transposed`` would build from the CSR arrays of M (``amdmsm_plan_fr_matrix_transposed``):
    ``plan_fr_matrix`` of the transpose, with the validation and the codes of the plain plan."""
    return _plan_fr_matrix("amdmsm_plan_fr_matrix_transposed", curve, offsets, cols, coeffs, n_cols, plain)


def _plan_fr_matrix(entry, curve, offsets, cols, coeffs, n_cols, plain):
    offsets, cols, coeffs, n_rows, ptr = _csr_arrays(curve, offsets, cols, coeffs)
    out = (ctypes.c_size_t * FR_MATRIX_PLAN_WORDS)()
    rc = getattr(load_library(), entry)(curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(offsets), ptr(cols),
                                        ptr(coeffs), int(plain), out)
    if rc:
        raise AmdMsmError(f"{entry}: {rc}")
    return {"nnz": out[0], "general": out[1], "plus_one": out[2], "minus_one": out[3], "zero": out[4],
            "rows_lane": out[5], "rows_wave": out[6], "rows_split": out[7], "wave_row": out[8], "split_row": out[9],
            "longest_row": out[10], "device_bytes": out[11], "launches": out[12], "chunk": out[13], "wave_jobs": out[14],
            "partials": out[15]}


class FrMatrix:
    """A sparse matrix over Fr resident on the device (``Engine.fr_matrix_load``); ``free()`` or a ``with`` block
    releases it, the engine's ``close()`` whatever is left."""

    def __init__(self, engine, handle, curve, n_rows, n_cols):
        self.engine, self.handle, self.curve, self.n_rows, self.n_cols = engine, handle, curve, n_rows, n_cols

    def free(self):
        if self.handle:
            h, self.handle = self.handle, 0
            self.engine._check(self.engine.lib.amdmsm_fr_matrix_free(self.engine.h, ctypes.c_uint64(h)), "amdmsm_fr_matrix_free")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _fr_record(x, limbs, r, plain):
    """the int ``x`` as one Fr record: plain, or libff's Montgomery residue with R = 2^(64 limbs)"""
    x = int(x) % r
    if not plain:
        x = x * (1 << (64 * limbs)) % r
    return np.frombuffer(x.to_bytes(8 * limbs, "little"), dtype="<u8").astype(np.uint64)


# include/amdmsm.h AMDMSM_SCAN_*
SCAN_REVERSE, SCAN_EXCLUSIVE = 1, 2
SCAN_KIND_A, SCAN_KIND_B, SCAN_KIND_INVERT = 0x100, 0x200, 0x400


def plan_fr_scan(curve, n, a=True, b=False, invert=False, reverse=False, exclusive=False, tile_log2=0):
    """What ``Engine.fr_scan`` (``a`` / ``b``: which operands are given) or ``Engine.fr_batch_invert`` (``invert``) runs
    for ``n`` records (``amdmsm_plan_fr_scan``, read-only, no device): records per tile and per lane, tiles per spine
    step, the range of ``tile_log2``, launches, workspace bytes and field products per record."""
    kind = SCAN_KIND_INVERT if invert else (SCAN_KIND_A if a else 0) | (SCAN_KIND_B if b else 0)
    kind |= (SCAN_REVERSE if reverse else 0) | (SCAN_EXCLUSIVE if exclusive else 0)
    out = (ctypes.c_size_t * 8)()
    rc = load_library().amdmsm_plan_fr_scan(curve, ctypes.c_size_t(n), kind, int(tile_log2), out)
    if rc:
        raise AmdMsmError(f"amdmsm_plan_fr_scan: {rc}")
    return {"tile": out[0], "per_lane": out[1], "spine_step": out[2], "tile_min": out[3], "tile_max": out[4],
            "launches": out[5], "workspace_bytes": out[6], "products_per_record": out[7]}


def fr_inverse(curve, x, plain=True):
    """``1 / x`` in Fr of the curve (``amdmsm_fr_inverse``: one Fermat power on the host), ``x`` and the result ints --
    with ``plain=False`` both are taken as Montgomery residues.  ValueError for 0 and for a value not below r."""
    limbs = _fr_limbs(curve)
    x = int(x)
    if x < 0 or x >> (64 * limbs):
        raise ValueError("x does not fit an Fr record")
    src = np.frombuffer(x.to_bytes(8 * limbs, "little"), dtype="<u8").astype(np.uint64)
    out = np.zeros(limbs, dtype=np.uint64)
    rc = load_library().amdmsm_fr_inverse(curve, _np_ptr(src), int(bool(plain)), _np_ptr(out))
    if rc:
        raise ValueError(f"amdmsm_fr_inverse: {rc} (x = 0 or x >= r)")
    return int.from_bytes(out.tobytes(), "little")


# include/amdmsm.h AMDMSM_DOMAIN_*
DOMAIN_BASIC_RADIX2, DOMAIN_STEP_RADIX2 = 0, 1
DOMAIN_INVERSE = 1


def _domain_error(what, rc):
    err = AmdMsmError(f"{what}: {rc}")
    err.code = rc   # the AMDMSM_ERR_* value of include/amdmsm.h
    return err


def fr_domain(curve, min_size):
    """The evaluation domain libfqfft's ``get_evaluation_domain(min_size)`` chooses over Fr of the curve
    (``amdmsm_fr_domain``, no device): ``kind`` (``DOMAIN_BASIC_RADIX2`` or ``DOMAIN_STEP_RADIX2``), its size ``m`` >=
    min_size, ``B`` and ``S`` (m = B + S for a step domain; B = m and S = 0 for a basic one), ``omega_log2`` (log2 of the
    order of the domain's root) and the workspace bytes of a device transform.  AmdMsmError with ``code`` -3 where
    libfqfft would use a domain that is left out, -5 above 2^28 points, -2 below 2."""
    out = (ctypes.c_size_t * 6)()
    rc = load_library().amdmsm_fr_domain(curve, ctypes.c_size_t(int(min_size) if min_size >= 0 else 0), out)
    if rc:
        raise _domain_error("amdmsm_fr_domain", rc)
    return {"kind": out[0], "m": out[1], "B": out[2], "S": out[3], "omega_log2": out[4], "workspace_bytes": out[5]}


def _fr_host_int(curve, x):
    limbs = _fr_limbs(curve)
    x = int(x)
    if x < 0 or x >> (64 * limbs):
        raise ValueError("the value does not fit an Fr record")
    return np.frombuffer(x.to_bytes(8 * limbs, "little"), dtype="<u8").astype(np.uint64)


def fr_domain_element(curve, m, idx, plain=True):
    """Element ``idx`` of the domain of ``m`` points (``amdmsm_fr_domain_element``), an int; ``plain=False``: its
    Montgomery residue."""
    out = np.zeros(_fr_limbs(curve), dtype=np.uint64)
    rc = load_library().amdmsm_fr_domain_element(curve, ctypes.c_size_t(m), ctypes.c_size_t(idx), int(bool(plain)), _np_ptr(out))
    if rc:
        raise _domain_error("amdmsm_fr_domain_element", rc)
    return int.from_bytes(out.tobytes(), "little")


def fr_domain_vanishing(curve, m, t, plain=True):
    """``Z(t)`` of the domain of ``m`` points (``amdmsm_fr_domain_vanishing``); ``t`` and the result ints in the form
    ``plain`` says."""
    src, out = _fr_host_int(curve, t), np.zeros(_fr_limbs(curve), dtype=np.uint64)
    rc = load_library().amdmsm_fr_domain_vanishing(curve, ctypes.c_size_t(m), _np_ptr(src), int(bool(plain)), _np_ptr(out))
    if rc:
        raise _domain_error("amdmsm_fr_domain_vanishing", rc)
    return int.from_bytes(out.tobytes(), "little")


def fr_domain_z_terms(curve, m, plain=True):
    """The vanishing polynomial of the domain of ``m`` points as a list of ``(index, coefficient)``, the highest index
    first (``amdmsm_fr_domain_z_terms``): two terms for a basic domain, four for a step domain."""
    limbs = _fr_limbs(curve)
    idx, coeffs, count = (ctypes.c_size_t * 4)(), np.zeros((4, limbs), dtype=np.uint64), ctypes.c_int(0)
    rc = load_library().amdmsm_fr_domain_z_terms(curve, ctypes.c_size_t(m), int(bool(plain)), idx, _np_ptr(coeffs), ctypes.byref(count))
    if rc:
        raise _domain_error("amdmsm_fr_domain_z_terms", rc)
    return [(int(idx[k]), int.from_bytes(coeffs[k].tobytes(), "little")) for k in range(count.value)]


def fr_multiplicative_generator(curve, plain=True):
    """libff's ``Fr::multiplicative_generator`` (``amdmsm_fr_multiplicative_generator``), an int: the coset shift of a
    quotient."""
    out = np.zeros(_fr_limbs(curve), dtype=np.uint64)
    rc = load_library().amdmsm_fr_multiplicative_generator(curve, int(bool(plain)), _np_ptr(out))
    if rc:
        raise _domain_error("amdmsm_fr_multiplicative_generator", rc)
    return int.from_bytes(out.tobytes(), "little")


def _fr_host_record(x, limbs, r, plain):
    """one host record of a scan: None, an int (reduced and put in the form ``plain`` says) or an array of fr_limbs
    words taken as it stands"""
    if x is None or isinstance(x, np.ndarray):
        return x if x is None else np.ascontiguousarray(x, dtype=np.uint64).reshape(limbs)
    return _fr_record(x, limbs, r, plain)


def endomorphism_info(curve, group):
    """lambda (int), log2 bound of the half scalars, whether the whole curve group has order r"""
    s = sizes(curve, group)
    lam = (ctypes.c_uint8 * s["fr_bytes"])()
    bound, prime = ctypes.c_int(0), ctypes.c_int(0)
    rc = load_library().amdmsm_endomorphism_info(curve, group, lam, ctypes.byref(bound), ctypes.byref(prime))
    if rc:
        raise AmdMsmError(f"amdmsm_endomorphism_info: {rc}")
    return {"lambda": int.from_bytes(bytes(lam), "little"), "bound_log2": bound.value / 1000.0,
            "prime_order": bool(prime.value)}


def multi_exp_multi(engines, curve, group, bases, scalars, base_form=multi_exp_base_form_normal,
                    out_form=OUT_AFFINE, window_bits=0, scalars_plain=False):
    """amdmsm_multi_exp_multi: libff's range split (multiexp.tcc:655-687) with chunk = engine context
    (one per GPU, or several on one GPU), partials combined on engines[0]'s device."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    s = sizes(curve, group)
    n = bases.shape[0] if bases.ndim == 2 else 0
    out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
    e0 = engines[0]
    ctxs = (ctypes.c_void_p * len(engines))(*[e.h for e in engines])
    o = e0._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
    rc = e0.lib.amdmsm_multi_exp_multi(ctxs, len(engines), curve, group, _np_ptr(bases) if n else None,
                                       ctypes.c_size_t(s["g_bytes"]), base_form, _np_ptr(scalars) if n else None,
                                       ctypes.c_size_t(n), _np_ptr(out), ctypes.byref(o))
    e0._check(rc, "amdmsm_multi_exp_multi")
    return out


def multi_exp_filter_one_zero_multi(engines, curve, group, bases, scalars, base_form=multi_exp_base_form_normal,
                                    out_form=OUT_AFFINE, window_bits=0, scalars_plain=False):
    """amdmsm_multi_exp_filter_one_zero_multi: (result, {"skipped", "ones", "other"}) with the range split of
    multi_exp_multi; every context counts the zeros / ones of its own range."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    s = sizes(curve, group)
    n = bases.shape[0] if bases.ndim == 2 else 0
    out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
    st = (ctypes.c_size_t * 3)()
    e0 = engines[0]
    ctxs = (ctypes.c_void_p * len(engines))(*[e.h for e in engines])
    o = e0._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
    rc = e0.lib.amdmsm_multi_exp_filter_one_zero_multi(ctxs, len(engines), curve, group, _np_ptr(bases) if n else None,
                                                       ctypes.c_size_t(s["g_bytes"]), base_form,
                                                       _np_ptr(scalars) if n else None, ctypes.c_size_t(n), _np_ptr(out),
                                                       ctypes.byref(o), st)
    e0._check(rc, "amdmsm_multi_exp_filter_one_zero_multi")
    return out, {"skipped": st[0], "ones": st[1], "other": st[2]}


def msm_device_multi(engines, curve, group, d_bases, d_scalars, counts, d_out_dev0, out_form=OUT_LIBFF, window_bits=0,
                     scalars_plain=False, stream=None):
    """amdmsm_msm_device_multi: range k (compact affine bases, scalars; device pointers on
    engines[k]'s GPU) is reduced there, the partials are summed on engines[0]'s GPU into d_out_dev0."""
    k = len(engines)
    e0 = engines[0]
    ctxs = (ctypes.c_void_p * k)(*[e.h for e in engines])
    pb = (ctypes.c_void_p * k)(*[_vp(x) for x in d_bases])
    ps = (ctypes.c_void_p * k)(*[_vp(x) for x in d_scalars])
    cn = (ctypes.c_size_t * k)(*counts)
    o = e0._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain, stream=stream)
    rc = e0.lib.amdmsm_msm_device_multi(ctxs, k, curve, group, pb, ps, cn, _vp(d_out_dev0), ctypes.byref(o))
    e0._check(rc, "amdmsm_msm_device_multi")


def _vp(x):
    """device address (int, e.g. torch's data_ptr()) or c_void_p (Engine.malloc) -> c_void_p"""
    return x if isinstance(x, ctypes.c_void_p) else ctypes.c_void_p(x)


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _opt_ptr(a):
    return None if a is None else _np_ptr(a)   # a host array that may be absent


def _opt_dev(p):
    return None if p is None else _vp(p)   # a device address that may be absent


def _fr_limbs(curve):
    return sizes(curve, G1)["fr_bytes"] // 8


def _fr_array(curve, a):
    """``a`` as a contiguous (n, fr_limbs) uint64 array, and its n; None stays None, with n = 0"""
    a = None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, _fr_limbs(curve))
    return a, 0 if a is None else a.shape[0]


# include/amdmsm.h amdmsm_read_fn: size_t read(void *read_ctx, void *dst, size_t bytes)
_READ_FN = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
# include/amdmsm.h amdmsm_write_fn: size_t write(void *write_ctx, const void *src, size_t bytes)
_WRITE_FN = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


def plan_write_points(n, chunk_points=0):
    """The chunks of ``Engine.write_points_stream`` / ``write_points_file`` over ``n`` records
    (``amdmsm_plan_write_points``, no device): a list of ``(first record, records, staging buffer)``."""
    lib, out, chunks = load_library(), (ctypes.c_size_t * 4)(), []
    k = 0
    while True:
        rc = lib.amdmsm_plan_write_points(ctypes.c_size_t(n), ctypes.c_size_t(chunk_points), ctypes.c_size_t(k), out)
        if rc:
            raise AmdMsmError(f"amdmsm_plan_write_points: {rc}")
        if k >= out[0]:
            return chunks
        chunks.append((int(out[1]), int(out[2]), int(out[3])))
        k += 1


def _records(a, stride_bytes, g_bytes):
    """libff records in the array ``a``, ``stride_bytes`` apart (None: the rows of a packed 2-d array)"""
    if stride_bytes is None:
        return int(a.shape[0]) if a.ndim == 2 else 0
    return (a.nbytes - g_bytes) // stride_bytes + 1 if a.nbytes >= g_bytes else 0


def _result_array(out, rows, g_bytes):
    """``out``, or a fresh array when the caller gave none: ``rows`` libff records"""
    if out is None:
        out = np.zeros((rows, g_bytes // 8), dtype=np.uint64)
    assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (rows, g_bytes // 8)
    return out


class Engine:
    """One amdmsm context (device, stream, workspace).  Fails loudly without a GPU."""

    def __init__(self, device=0, endomorphism=0):
        self.lib = load_library()
        self.device = device
        self.endomorphism = endomorphism
        h = ctypes.c_void_p()
        rc = self.lib.amdmsm_ctx_create(device, ctypes.byref(h))
        if rc:
            raise AmdMsmError("amdmsm_ctx_create(device=%d) failed: %s" %
                              (device, self.lib.amdmsm_strerror(rc).decode()))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.amdmsm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            err = AmdMsmError("%s failed: %s (%s)" % (what, self.lib.amdmsm_strerror(rc).decode(),
                                                      self.lib.amdmsm_last_error(self.h).decode()))
            err.code = rc   # the AMDMSM_ERR_* value of include/amdmsm.h
            raise err

    def _opts(self, window_bits=0, segment_len=0, out_form=OUT_LIBFF, scalars_plain=False, stream=None):
        # self.endomorphism: amdmsm_opts.endomorphism for every call of this engine (0 = only where the
        # whole curve group has order r, 1 = the bases are promised to lie in the order-r subgroup, -1 = off)
        return _Opts(ctypes.sizeof(_Opts), window_bits, segment_len, out_form, int(scalars_plain), int(self.endomorphism),
                     stream)

    # ---------------------------------------------------------------- host API
    def multi_exp(self, curve, group, bases, scalars, method=multi_exp_method_BDLO12_signed,
                  base_form=multi_exp_base_form_normal, chunks=1, out_form=OUT_AFFINE, window_bits=0,
                  scalars_plain=False, split_chunks=False):
        """libff::multi_exp<G, Fr, Method, BaseForm>(bases, scalars, chunks), multiexp.tcc:643-688.

        BDLO12 and BDLO12_signed both run the device Pippenger engine (the result is a
        group element; it does not depend on the digit convention).  ``chunks`` is the
        reference's CPU-thread hint (libsnark passes its OpenMP thread count): one GPU runs the
        whole input as ONE MSM whatever its value -- splitting would only multiply the fixed
        costs -- and across GPUs the split is ``multi_exp_multi``'s.  ``split_chunks=True``
        forces the reference's split-and-sum shape (contiguous ranges, the last one takes the
        remainder, partials summed; multiexp.tcc:655-687) on this one device, for the parity tests
        of range sharding.
        """
        if method not in (multi_exp_method_BDLO12, multi_exp_method_BDLO12_signed):
            raise NotImplementedError("only the BDLO12 / BDLO12_signed methods run on the GPU engine")
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        n = bases.shape[0] if bases.ndim == 2 else 0
        if n:
            assert bases.shape[1] * 8 == s["g_bytes"], "bases must be (n, 3*coord_limbs) uint64"
            assert scalars.shape == (n, s["fr_bytes"] // 8), "scalars must be (n, fr_limbs) uint64"
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        total = n
        if total < chunks or chunks == 1 or not split_chunks:
            o = self._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
            rc = self.lib.amdmsm_multi_exp(self.h, curve, group, _np_ptr(bases) if n else None,
                                           ctypes.c_size_t(s["g_bytes"]), base_form,
                                           _np_ptr(scalars) if n else None, ctypes.c_size_t(n), _np_ptr(out),
                                           ctypes.byref(o))
            self._check(rc, "amdmsm_multi_exp")
            return out
        one = total // chunks
        partials = np.zeros((chunks, s["g_bytes"] // 8), dtype=np.uint64)
        o = self._opts(window_bits=window_bits, out_form=OUT_JACOBIAN, scalars_plain=scalars_plain)
        for i in range(chunks):
            lo = i * one
            hi = total if i == chunks - 1 else (i + 1) * one
            b, sc = bases[lo:hi], scalars[lo:hi]
            rc = self.lib.amdmsm_multi_exp(self.h, curve, group, _np_ptr(b), ctypes.c_size_t(s["g_bytes"]),
                                           base_form, _np_ptr(sc), ctypes.c_size_t(hi - lo),
                                           _np_ptr(partials[i]), ctypes.byref(o))
            self._check(rc, "amdmsm_multi_exp")
        return self.sum_points(curve, group, partials, out_form=out_form)

    def multi_exp_short(self, curve, group, bases, scalars, bits=0, base_form=multi_exp_base_form_normal,
                        out_form=OUT_AFFINE, window_bits=0, scalars_plain=False):
        """``multi_exp`` for scalars known to be short (``amdmsm_multi_exp_short``).  A one-dimensional array of dtype
        uint8 / uint16 / uint32 / uint64 is passed as packed integers (``n * width`` bytes are uploaded); an
        ``(n, fr_limbs)`` uint64 array is passed as Fr records.  ``bits``: 0 = the kind's full width, N > 0 = the
        promise that every scalar is below ``2**N`` (a broken promise raises, nothing is returned), -1 = measure on the
        device first."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        scalars = np.ascontiguousarray(scalars)
        s = sizes(curve, group)
        n = bases.shape[0] if bases.ndim == 2 else 0
        if scalars.ndim == 1 and scalars.dtype.name in _INT_KINDS:
            kind = _INT_KINDS[scalars.dtype.name]
            assert scalars.shape[0] == n, "one scalar per base"
        else:
            kind = SCALAR_FR
            scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
            if n:
                assert scalars.shape == (n, s["fr_bytes"] // 8), "scalars must be (n, fr_limbs) uint64 or a packed integer vector"
        if n:
            assert bases.shape[1] * 8 == s["g_bytes"], "bases must be (n, 3*coord_limbs) uint64"
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        o = self._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
        d = scalar_desc(kind, bits)
        rc = self.lib.amdmsm_multi_exp_short(self.h, curve, group, _np_ptr(bases) if n else None,
                                             ctypes.c_size_t(s["g_bytes"]), base_form, _np_ptr(scalars) if n else None,
                                             ctypes.byref(d), ctypes.c_size_t(n), _np_ptr(out), ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_short")
        return out

    def multi_exp_batch(self, curve, group, bases_list, scalars_list, base_form=multi_exp_base_form_normal,
                        out_form=OUT_AFFINE, window_bits=0, scalars_plain=False):
        """amdmsm_multi_exp_batch: len(bases_list) multi_exp calls of one group and length as one batch; list of results."""
        k = len(bases_list)
        bs = [np.ascontiguousarray(b, dtype=np.uint64) for b in bases_list]
        ss = [np.ascontiguousarray(x, dtype=np.uint64) for x in scalars_list]
        s = sizes(curve, group)
        n = bs[0].shape[0]
        assert all(b.shape == bs[0].shape for b in bs) and all(x.shape[0] == n for x in ss)
        outs = [np.zeros(s["g_bytes"] // 8, dtype=np.uint64) for _ in range(k)]
        pb = (ctypes.c_void_p * k)(*[_np_ptr(b) for b in bs])
        ps = (ctypes.c_void_p * k)(*[_np_ptr(x) for x in ss])
        po = (ctypes.c_void_p * k)(*[_np_ptr(o) for o in outs])
        o = self._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_batch(self.h, curve, group, k, pb, ctypes.c_size_t(s["g_bytes"]), base_form, ps,
                                             ctypes.c_size_t(n), po, ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_batch")
        return outs

    def multi_exp_batch_items(self, curve, group, items, shared_scalars=None, base_form=multi_exp_base_form_normal,
                              out_form=OUT_AFFINE, window_bits=0, scalars_plain=False):
        """amdmsm_multi_exp_batch_items: up to 8 multi_exp calls of one group, each of its own length, as one batch.

        ``items``: ``BatchItem`` objects or dicts with ``bases`` and one of ``scalars`` / ``offset`` / ``index``.  Items
        without ``scalars`` take theirs from ``shared_scalars`` (uploaded once), selected on the device.  ``bases`` that
        were registered must be passed as the very arrays (or row ranges of them).  Returns the list of results.
        """
        its = [BatchItem(**it) if isinstance(it, dict) else it for it in items]
        k = len(its)
        s = sizes(curve, group)
        fr_limbs = s["fr_bytes"] // 8
        shared = None if shared_scalars is None else np.ascontiguousarray(shared_scalars, dtype=np.uint64)
        shared_n = 0 if shared is None else shared.shape[0]
        if shared is not None and shared_n:
            assert shared.shape == (shared_n, fr_limbs), "shared_scalars must be (shared_n, fr_limbs) uint64"
        arr = (BatchItemStruct * max(k, 1))()
        keep, outs = [], []
        for j, it in enumerate(its):
            b = np.ascontiguousarray(it.bases, dtype=np.uint64)   # (a contiguous uint64 array is passed through as it is)
            n = b.shape[0] if b.ndim == 2 else 0
            if n:
                assert b.shape[1] * 8 == s["g_bytes"], "bases must be (n, 3*coord_limbs) uint64"
            out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
            sc = idx = None
            if it.scalars is not None:
                sc = np.ascontiguousarray(it.scalars, dtype=np.uint64)
                assert n == 0 or sc.shape == (n, fr_limbs), "scalars must be (n, fr_limbs) uint64"
            if it.index is not None:
                idx = np.ascontiguousarray(it.index, dtype=np.uint32)
                assert idx.shape == (n,), "index must hold one uint32 per base"
            keep += [b, sc, idx]
            outs.append(out)
            arr[j] = BatchItemStruct(ctypes.sizeof(BatchItemStruct), _np_ptr(b) if n else None, n,
                                     _np_ptr(sc) if sc is not None and n else None, int(it.offset),
                                     _np_ptr(idx) if idx is not None and n else None, _np_ptr(out))
        o = self._opts(window_bits=window_bits, out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_batch_items(self.h, curve, group, k, arr, ctypes.c_size_t(s["g_bytes"]), base_form,
                                                   _np_ptr(shared) if shared_n else None, ctypes.c_size_t(shared_n),
                                                   ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_batch_items")
        return outs

    def register_bases(self, curve, group, bases, base_form=multi_exp_base_form_normal):
        """amdmsm_register_bases: keep ``bases`` (the very numpy buffer -- the registry is keyed on its
        address) resident in HBM; later host-buffer calls on it or on row ranges of it skip the base
        transfer and import.  Returns a handle for ``unregister_bases``."""
        assert bases.dtype == np.uint64 and bases.flags["C_CONTIGUOUS"]
        s = sizes(curve, group)
        h = ctypes.c_uint64(0)
        rc = self.lib.amdmsm_register_bases(self.h, curve, group, _np_ptr(bases), ctypes.c_size_t(s["g_bytes"]),
                                            base_form, ctypes.c_size_t(bases.shape[0]), ctypes.byref(h))
        self._check(rc, "amdmsm_register_bases")
        return h.value

    def unregister_bases(self, handle):
        self._check(self.lib.amdmsm_unregister_bases(self.h, ctypes.c_uint64(handle)), "amdmsm_unregister_bases")

    def invalidate_bases(self, arr=None):
        rc = self.lib.amdmsm_invalidate_bases(self.h, _np_ptr(arr) if arr is not None else None,
                                              ctypes.c_size_t(arr.nbytes if arr is not None else 0))
        self._check(rc, "amdmsm_invalidate_bases")

    def multi_exp_filter_one_zero(self, curve, group, bases, scalars, method=multi_exp_method_BDLO12_signed,
                                  base_form=multi_exp_base_form_normal, chunks=1, out_form=OUT_AFFINE,
                                  scalars_plain=False):
        """libff::multi_exp_filter_one_zero, multiexp.tcc:690-757.  Returns (result, stats)."""
        if method not in (multi_exp_method_BDLO12, multi_exp_method_BDLO12_signed):
            raise NotImplementedError("only the BDLO12 / BDLO12_signed methods run on the GPU engine")
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        n = bases.shape[0]
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        stats = (ctypes.c_size_t * 3)()
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_filter_one_zero(
            self.h, curve, group, _np_ptr(bases), ctypes.c_size_t(s["g_bytes"]), base_form, _np_ptr(scalars),
            ctypes.c_size_t(n), _np_ptr(out), ctypes.byref(o), stats)
        self._check(rc, "amdmsm_multi_exp_filter_one_zero")
        return out, {"skipped": stats[0], "ones": stats[1], "other": stats[2]}

    def batch_to_special(self, curve, group, elems):
        """libff::batch_to_special<G>, multiexp.tcc:949-974 (returns a converted copy)."""
        elems = np.ascontiguousarray(elems, dtype=np.uint64).copy()
        s = sizes(curve, group)
        rc = self.lib.amdmsm_batch_to_special(self.h, curve, group, _np_ptr(elems), ctypes.c_size_t(s["g_bytes"]),
                                              ctypes.c_size_t(elems.shape[0]))
        self._check(rc, "amdmsm_batch_to_special")
        return elems

    def multi_exp_stream_file(self, curve, group, path, scalars, offset_bytes=0, chunk_points=0,
                              out_form=OUT_AFFINE, scalars_plain=False):
        """libff::multi_exp_stream<form_montgomery, compression_off> (multiexp_stream.tcc:164-191) with
        the base elements read from ``path`` in libff's on-disk format."""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_stream_file(self.h, curve, group, path.encode(), ctypes.c_size_t(offset_bytes),
                                                   _np_ptr(scalars) if scalars.shape[0] else None,
                                                   ctypes.c_size_t(scalars.shape[0]), ctypes.c_size_t(chunk_points),
                                                   _np_ptr(out), ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_stream_file")
        return out

    def multi_exp_stream_compressed_file(self, curve, group, path, scalars, offset_bytes=0, chunk_points=0,
                                         out_form=OUT_AFFINE, scalars_plain=False):
        """libff::multi_exp_stream<form_montgomery, compression_on>: ``path`` holds compressed records
        (curve_serialization.tcc:103-133); Y is recovered on the device."""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_stream_compressed_file(
            self.h, curve, group, path.encode(), ctypes.c_size_t(offset_bytes),
            _np_ptr(scalars) if scalars.shape[0] else None, ctypes.c_size_t(scalars.shape[0]),
            ctypes.c_size_t(chunk_points), _np_ptr(out), ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_stream_compressed_file")
        return out

    def disk_decode(self, curve, group, records, n, compressed):
        """group_read<encoding_binary, form_montgomery, compression_{off,on}> of ``n`` records (uint8 array)
        on the device -> (special-form (X, Y, Z) records, status)."""
        records = np.ascontiguousarray(records, dtype=np.uint8)
        s = sizes(curve, group)
        d_rec, d_aff, d_xyz = self.malloc(max(16, records.nbytes)), self.malloc(max(16, n * s["affine_bytes"])), \
            self.malloc(max(16, n * s["g_bytes"]))
        try:
            self.h2d(d_rec, records)
            st = ctypes.c_uint(0)
            self._check(self.lib.amdmsm_disk_decode_device(self.h, curve, group, d_rec, ctypes.c_size_t(n), int(compressed),
                                                           d_aff, ctypes.byref(st)), "amdmsm_disk_decode_device")
            self.export_affine_device(curve, group, d_aff.value, n, d_xyz.value)
            out = np.zeros((n, s["g_bytes"] // 8), dtype=np.uint64)
            self.synchronize()
            self.d2h(out, d_xyz)
            return out, st.value
        finally:
            for p in (d_rec, d_aff, d_xyz):
                self.free(p)

    def disk_encode_device(self, curve, group, d_points_affine, n, d_records, compressed=False, stream=None):
        """group_write<encoding_binary, form_montgomery, compression_{off,on}> of ``n`` compact affine points in HBM
        (``amdmsm_disk_encode_device``): ``n`` records to ``d_records``; enqueued on ``stream``, not synchronised."""
        self._check(self.lib.amdmsm_disk_encode_device(self.h, curve, group, _opt_dev(d_points_affine), ctypes.c_size_t(n),
                                                       int(compressed), _opt_dev(d_records), _vp(stream)),
                    "amdmsm_disk_encode_device")

    def disk_encode(self, curve, group, points_xyz, compressed=False, base_form=multi_exp_base_form_normal):
        """The twin of ``disk_decode``: (n, 3 * coordinate limbs) libff records in ``base_form`` -> their on-disk records
        as a uint8 array, encoded on the device."""
        pts = np.ascontiguousarray(points_xyz, dtype=np.uint64)
        s = sizes(curve, group)
        n = pts.shape[0] if pts.ndim == 2 else 0
        rec = s["affine_bytes"] // 2 if compressed else s["affine_bytes"]
        out = np.zeros(n * rec, dtype=np.uint8)
        d_xyz, d_aff, d_rec = self.malloc(max(16, pts.nbytes)), self.malloc(max(16, n * s["affine_bytes"])), \
            self.malloc(max(16, n * rec))
        try:
            if n:
                assert pts.shape[1] * 8 == s["g_bytes"], "points must be (n, 3*coord_limbs) uint64"
                self.h2d(d_xyz, pts)
                self.import_bases_device(curve, group, d_xyz, s["g_bytes"], base_form, n, d_aff)
            self.disk_encode_device(curve, group, d_aff, n, d_rec, compressed)
            self.synchronize()
            if n:
                self.d2h(out, d_rec)
            return out
        finally:
            for p in (d_xyz, d_aff, d_rec):
                self.free(p)

    def write_points_file(self, curve, group, d_points_affine, n, path, offset_bytes=0, compressed=False, chunk_points=0):
        """``n`` compact affine points in HBM into ``path`` as libff's on-disk records (``amdmsm_write_points_file``), from
        ``offset_bytes`` on; the file is not truncated.  What ``multi_exp_stream_file`` and its siblings read."""
        self._check(self.lib.amdmsm_write_points_file(self.h, curve, group, _opt_dev(d_points_affine), ctypes.c_size_t(n),
                                                      int(compressed), os.fsencode(path), ctypes.c_size_t(offset_bytes),
                                                      ctypes.c_size_t(chunk_points)), "amdmsm_write_points_file")

    def write_points_stream(self, curve, group, d_points_affine, n, writer, compressed=False, chunk_points=0):
        """The same records through ``writer.write(bytes)`` (``amdmsm_write_points_stream``): one call per chunk of
        ``chunk_points`` records, in order.  A ``write`` that returns a number below the length it was given ends the
        call (AmdMsmError); one that returns None has taken everything.  An exception raised by ``writer`` ends the call
        and is raised again after it."""
        raised = []

        def write(_ctx, src, nbytes):
            try:
                took = writer.write(ctypes.string_at(src, nbytes))
                return int(nbytes) if took is None else max(0, min(int(took), int(nbytes)))
            except BaseException as e:   # an exception cannot cross the C frames: end the call, raise afterwards
                raised.append(e)
                return 0

        cb = _WRITE_FN(write)   # referenced from this frame for as long as the library may call it
        rc = self.lib.amdmsm_write_points_stream(self.h, curve, group, _opt_dev(d_points_affine), ctypes.c_size_t(n),
                                                 int(compressed), cb, None, ctypes.c_size_t(chunk_points))
        del cb
        if raised:
            raise raised[0]
        self._check(rc, "amdmsm_write_points_stream")

    def batch_exp_device(self, curve, group, scalar_size, window, g, d_scalars, n, d_out_xyz, coeff=None,
                         scalars_plain=False, out_form=OUT_LIBFF, stream=None):
        """``batch_exp`` on ``n`` device-resident scalars, the results left at ``d_out_xyz`` (``amdmsm_batch_exp_device``);
        ``g`` and ``coeff`` are host arrays.  Shares the resident window table with ``batch_exp``; enqueued on
        ``stream``, not synchronised (``batch_exp_timings`` waits for it)."""
        g = None if g is None else np.ascontiguousarray(g, dtype=np.uint64)
        cf = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.uint64)
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain, stream=stream)
        self._check(self.lib.amdmsm_batch_exp_device(self.h, curve, group, ctypes.c_size_t(scalar_size), ctypes.c_size_t(window),
                                                     _opt_ptr(g), _opt_dev(d_scalars), ctypes.c_size_t(n), _opt_ptr(cf),
                                                     _opt_dev(d_out_xyz), ctypes.byref(o)), "amdmsm_batch_exp_device")

    def multi_exp_stream_with_precompute_file(self, curve, group, path, scalars, precompute_c, offset_bytes=0,
                                              chunk_points=0, out_form=OUT_AFFINE, scalars_plain=False):
        """libff::multi_exp_stream_with_precompute<form_montgomery, compression_off>
        (multiexp_stream.tcc:193-223): ``path`` holds precompute_num_digits(curve, c) multiples
        [2^(jc)]P per base, as profile_multiexp.cpp:120-150 writes them."""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_multi_exp_stream_with_precompute_file(
            self.h, curve, group, path.encode(), ctypes.c_size_t(offset_bytes),
            _np_ptr(scalars) if scalars.shape[0] else None, ctypes.c_size_t(scalars.shape[0]),
            ctypes.c_size_t(precompute_c), ctypes.c_size_t(chunk_points), _np_ptr(out), ctypes.byref(o))
        self._check(rc, "amdmsm_multi_exp_stream_with_precompute_file")
        return out

    def multi_exp_stream(self, curve, group, reader, scalars, *, chunk_points=0, compressed=False, precompute_c=0,
                         out=None, out_form=OUT_AFFINE, scalars_plain=False):
        """The reader-callback entries ``amdmsm_multi_exp_stream`` / ``_compressed`` / ``_with_precompute`` (what the
        C++ shim of include/libff_amd/multiexp_stream.hpp calls): the records of the ``_file`` methods above, pulled
        through ``reader(nbytes) -> bytes``.  A reader may deliver fewer bytes than asked for (it is asked again for the
        rest, never for more than the call still needs); ``b""`` is the end of the stream.  ``compressed``: compressed
        records; ``precompute_c`` > 0: precompute_num_digits(curve, c) multiples per scalar.  ``out``: result record to
        fill; it is written only when the call succeeds.  An exception raised by ``reader`` ends the stream and is
        raised again after the call."""
        assert not (compressed and precompute_c), "the reference has no compressed precompute stream"
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        s = sizes(curve, group)
        if out is None:
            out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.nbytes == s["g_bytes"]
        raised = []

        def read(_ctx, dst, nbytes):
            try:
                piece = bytes(reader(int(nbytes)))
                assert len(piece) <= nbytes, "reader returned more than it was asked for"
                ctypes.memmove(dst, piece, len(piece))
                return len(piece)
            except BaseException as e:   # an exception cannot cross the C frames: end the stream, raise afterwards
                raised.append(e)
                return 0

        cb = _READ_FN(read)   # referenced from this frame for as long as the library may call it
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        n = scalars.shape[0]
        args = (_np_ptr(scalars) if n else None, ctypes.c_size_t(n))
        tail = (ctypes.c_size_t(chunk_points), _np_ptr(out), ctypes.byref(o))
        if precompute_c:
            what = "amdmsm_multi_exp_stream_with_precompute"
            rc = self.lib.amdmsm_multi_exp_stream_with_precompute(self.h, curve, group, cb, None, *args,
                                                                  ctypes.c_size_t(precompute_c), *tail)
        elif compressed:
            what = "amdmsm_multi_exp_stream_compressed"
            rc = self.lib.amdmsm_multi_exp_stream_compressed(self.h, curve, group, cb, None, *args, *tail)
        else:
            what = "amdmsm_multi_exp_stream"
            rc = self.lib.amdmsm_multi_exp_stream(self.h, curve, group, cb, None, *args, *tail)
        del cb
        if raised:
            raise raised[0]
        self._check(rc, what)
        return out

    def precompute_table(self, curve, group, bases, c, num_digits=None):
        """Host convenience around amdmsm_precompute_bases_device: special-form (x, y, 1) records in,
        table[i * D + j] = [2^(jc)] bases[i] out, again as special-form records."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        n = bases.shape[0]
        D = num_digits or precompute_num_digits(curve, c)
        s = sizes(curve, group)
        d_src = self.malloc(max(bases.nbytes, 16))
        d_aff = self.malloc(max(n * s["affine_bytes"], 16))
        d_tab = self.malloc(max(n * D * s["affine_bytes"], 16))
        d_out = self.malloc(max(n * D * s["g_bytes"], 16))
        try:
            self.h2d(d_src, bases)
            self.import_bases_device(curve, group, d_src, bases.strides[0], multi_exp_base_form_special, n, d_aff)
            self._check(self.lib.amdmsm_precompute_bases_device(
                self.h, curve, group, _vp(d_aff), ctypes.c_size_t(n), ctypes.c_size_t(c),
                ctypes.c_size_t(D), _vp(d_tab), None), "amdmsm_precompute_bases_device")
            self.export_affine_device(curve, group, d_tab, n * D, d_out)
            out = np.zeros((n * D, s["g_bytes"] // 8), dtype=np.uint64)
            self.synchronize()
            self.d2h(out, d_out)
        finally:
            for p in (d_src, d_aff, d_tab, d_out):
                self.free(p)
        return out

    def batch_exp(self, curve, group, scalar_size, window, g, v, coeff=None, scalars_plain=False, out=None):
        """libff::batch_exp / batch_exp_with_coeff (multiexp.tcc:874-947) for the table that
        get_window_table(scalar_size, window, g) would build: res[i] = (coeff *) v[i] * g.
        out: result array to fill (n, 3 * coordinate limbs) -- a caller that repeats the call passes the same
        array again and spares the page faults of a fresh 100 MB allocation."""
        g = np.ascontiguousarray(g, dtype=np.uint64)
        v = np.ascontiguousarray(v, dtype=np.uint64)
        s = sizes(curve, group)
        n = v.shape[0]
        if out is None:
            out = np.zeros((n, s["g_bytes"] // 8), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (n, s["g_bytes"] // 8)
        cf = np.ascontiguousarray(coeff, dtype=np.uint64) if coeff is not None else None
        rc = self.lib.amdmsm_batch_exp(self.h, curve, group, ctypes.c_size_t(scalar_size), ctypes.c_size_t(window),
                                       _np_ptr(g), _np_ptr(v) if n else None, ctypes.c_size_t(n),
                                       _np_ptr(cf) if cf is not None else None, int(scalars_plain),
                                       _np_ptr(out) if n else None)
        self._check(rc, "amdmsm_batch_exp")
        return out

    def scalar_mul_vec(self, curve, group, points, scalars, base_form=multi_exp_base_form_normal, out_form=OUT_LIBFF,
                       scalars_plain=False, chunk_points=0, stride_bytes=None, out=None):
        """Element-wise scalar multiplication (``amdmsm_scalar_mul_vec``): ``out[i] = scalars[i] * points[i]``, what a
        host does with libff's ``operator*`` in a loop.  ``points``: (n, 3 * coordinate limbs) libff records in
        ``base_form``; ``scalars``: (n, fr_limbs) Montgomery residues, or with ``scalars_plain`` any integers of that
        width (values >= r included).  ``chunk_points``: elements worked through at a time, 0 = automatic.
        ``stride_bytes``: bytes between two records of ``points`` (default: packed).  ``out``: result array to fill."""
        s = sizes(curve, group)
        points = np.ascontiguousarray(points, dtype=np.uint64)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        n = scalars.shape[0]
        out = _result_array(out, n, s["g_bytes"])
        if n:
            assert scalars.shape == (n, s["fr_bytes"] // 8), "scalars must be (n, fr_limbs) uint64"
            if stride_bytes is None:
                assert points.shape == (n, s["g_bytes"] // 8), "points must be (n, 3*coord_limbs) uint64"
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_scalar_mul_vec(self.h, curve, group, _np_ptr(points) if n else None,
                                            ctypes.c_size_t(s["g_bytes"] if stride_bytes is None else stride_bytes), base_form,
                                            _np_ptr(scalars) if n else None, ctypes.c_size_t(n), _np_ptr(out) if n else None,
                                            ctypes.c_size_t(chunk_points), ctypes.byref(o))
        self._check(rc, "amdmsm_scalar_mul_vec")
        return out

    def multi_exp_segments(self, curve, group, bases, scalars, offsets, *, shared_bases=False, long_from=0,
                           base_form=multi_exp_base_form_normal, out_form=OUT_LIBFF, scalars_plain=False, chunk_terms=0,
                           stride_bytes=None, out=None):
        """Segmented MSM (``amdmsm_multi_exp_segments``): ``out[j] = sum(scalars[i] * bases[i])`` over
        ``offsets[j] <= i < offsets[j + 1]``, ``len(offsets) - 1`` results from one call.  ``bases``: (n, 3 * coordinate
        limbs) libff records in ``base_form``; ``scalars``: (n_terms, fr_limbs) Montgomery residues, or with
        ``scalars_plain`` any integers of that width; ``offsets``: non-decreasing, ``offsets[-1] <= n_terms``.
        ``shared_bases``: term i of segment j uses ``bases[i - offsets[j]]`` (one query for every segment).  ``long_from``:
        segments of at least this many terms take the single-MSM route (0 = the library's default, ``SEG_LONG_NEVER``).
        ``chunk_terms``: terms worked through at a time, 0 = automatic.  ``stride_bytes``: bytes between two records of
        ``bases`` (default: packed).  ``out``: result array to fill."""
        s = sizes(curve, group)
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        m = max(int(offs.shape[0]) - 1, 0)
        n_terms = int(scalars.shape[0])
        n_bases = _records(bases, stride_bytes, s["g_bytes"])
        out = _result_array(out, m, s["g_bytes"])
        if n_terms:
            assert scalars.shape == (n_terms, s["fr_bytes"] // 8), "scalars must be (n_terms, fr_limbs) uint64"
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        self._check(self.lib.amdmsm_set_segments_chunk_terms(self.h, ctypes.c_size_t(chunk_terms)),
                    "amdmsm_set_segments_chunk_terms")
        try:
            rc = self.lib.amdmsm_multi_exp_segments(
                self.h, curve, group, _np_ptr(bases) if n_bases else None,
                ctypes.c_size_t(s["g_bytes"] if stride_bytes is None else stride_bytes), base_form, ctypes.c_size_t(n_bases),
                _np_ptr(scalars) if n_terms else None, ctypes.c_size_t(n_terms), _np_ptr(offs) if offs.shape[0] else None,
                ctypes.c_size_t(m), ctypes.c_uint(SEG_SHARED_BASES if shared_bases else 0), ctypes.c_size_t(long_from),
                _np_ptr(out) if m else None, ctypes.byref(o))
        finally:
            self.lib.amdmsm_set_segments_chunk_terms(self.h, ctypes.c_size_t(0))
        self._check(rc, "amdmsm_multi_exp_segments")
        return out

    def fold_vec(self, curve, group, points_list, scalars, base_form=multi_exp_base_form_normal, out_form=OUT_LIBFF,
                 scalars_plain=False, chunk_points=0, stride_bytes=None, out=None):
        """Fold of point vectors (``amdmsm_fold_vec``): ``out[i] = sum_j scalars[j] * points_list[j][i]``, k = 1 .. 8
        vectors of one length and k scalars shared by all elements.  ``points_list``: k arrays of (n, 3 * coordinate
        limbs) libff records in ``base_form`` (views of one array are fine); ``scalars``: (k, fr_limbs) Montgomery
        residues, or with ``scalars_plain`` any integers of that width.  The endomorphism split follows
        ``self.endomorphism`` (``plan_fold`` tells).  ``chunk_points``: elements worked through at a time, 0 = automatic.
        ``stride_bytes``: bytes between two records of every vector (default: packed).  ``out``: result array to fill."""
        s = sizes(curve, group)
        gl = s["g_bytes"] // 8
        vecs = [np.ascontiguousarray(p, dtype=np.uint64) for p in points_list]
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        k = len(vecs)
        n = _records(vecs[0], stride_bytes, s["g_bytes"]) if k else 0
        out = _result_array(out, n, s["g_bytes"])
        if n:
            assert scalars.shape == (k, s["fr_bytes"] // 8), "scalars must be (k, fr_limbs) uint64"
            for v in vecs:
                assert v.nbytes == vecs[0].nbytes, "the vectors must have one length"
                if stride_bytes is None:
                    assert v.shape == (n, gl), "every vector must be (n, 3*coord_limbs) uint64"
        ptrs = (ctypes.c_void_p * max(k, 1))(*[_np_ptr(v) if n else None for v in vecs])
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_fold_vec(self.h, curve, group, k, ptrs,
                                      ctypes.c_size_t(s["g_bytes"] if stride_bytes is None else stride_bytes), base_form,
                                      _np_ptr(scalars) if n else None, ctypes.c_size_t(n), _np_ptr(out) if n else None,
                                      ctypes.c_size_t(chunk_points), ctypes.byref(o))
        self._check(rc, "amdmsm_fold_vec")
        return out

    def group_fft(self, curve, group, points, twiddles, base_form=multi_exp_base_form_normal, out_form=OUT_LIBFF,
                  scalars_plain=False, chunk_points=0, stride_bytes=None, out=None):
        """Radix-2 FFT over a point vector (``amdmsm_group_fft``): ``out[j] = sum_i w^(i j) * points[i]``, n a power of
        two.  ``points``: (n, 3 * coordinate limbs) libff records in ``base_form``; ``twiddles``: (n / 2, fr_limbs) powers
        w^0 .. w^(n/2 - 1) of a primitive n-th root of unity, Montgomery residues or, with ``scalars_plain``, plain integers
        (``fft_twiddles`` makes those); None will do for n <= 2.  The inverse transform: the powers of w^-1, then
        ``fold_vec`` with k = 1 and the scalar n^-1.  ``chunk_points``: butterflies worked through at a time, 0 =
        automatic (``plan_group_fft`` tells).  ``stride_bytes``: bytes between two records of ``points`` (default:
        packed).  ``out``: result array to fill."""
        s = sizes(curve, group)
        gl = s["g_bytes"] // 8
        points = np.ascontiguousarray(points, dtype=np.uint64)
        n = _records(points, stride_bytes, s["g_bytes"])
        tw = None if twiddles is None else np.ascontiguousarray(twiddles, dtype=np.uint64)
        out = _result_array(out, n, s["g_bytes"])
        if n and stride_bytes is None:
            assert points.shape == (n, gl), "points must be (n, 3*coord_limbs) uint64"
        if tw is not None and tw.size:
            assert tw.shape == (n // 2, s["fr_bytes"] // 8), "twiddles must be (n / 2, fr_limbs) uint64"
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain)
        rc = self.lib.amdmsm_group_fft(self.h, curve, group, _np_ptr(points) if n else None,
                                       ctypes.c_size_t(s["g_bytes"] if stride_bytes is None else stride_bytes), base_form,
                                       ctypes.c_size_t(n), _np_ptr(tw) if tw is not None and tw.size else None,
                                       _np_ptr(out) if n else None, ctypes.c_size_t(chunk_points), ctypes.byref(o))
        self._check(rc, "amdmsm_group_fft")
        return out

    def _fr_params(self, curve, n, omega, inverse, coset, plain, given=(None, None, None)):
        """(omega, pre, post, scale) records of a transform of ``n`` scalars; the inverses are Python's.  ``given``: the
        caller's own (pre, post, scale) of the general form, each taking the place of the derived one"""
        r = fr_modulus(curve, G1)
        limbs = _fr_limbs(curve)
        w = (fr_root_of_unity(curve, n) if omega is None else int(omega)) if n > 1 else None
        pre = post = scale = None
        if inverse:
            w = None if w is None else pow(w, -1, r)
            scale = pow(n, -1, r) if n else None
            post = None if coset is None else pow(int(coset), -1, r)
        elif coset is not None:
            pre = int(coset)
        pre, post, scale = [d if g is None else int(g) for d, g in zip((pre, post, scale), given)]
        return [None if x is None else _fr_record(x, limbs, r, plain) for x in (w, pre, post, scale)]

    def fr_fft(self, curve, values, omega=None, inverse=False, coset=None, plain=False, tile_log2=0, out=None, *,
               pre=None, post=None, scale=None):
        """Radix-2 FFT over a vector of Fr scalars (``amdmsm_fr_fft``): ``out[j] = sum_i values[i] w^(i j)``, n a power
        of two, natural order in and out.  ``values``: (n, fr_limbs) uint64 Montgomery residues, with ``plain`` plain
        integers.  ``omega`` (an int): a primitive n-th root of unity, None = ``fr_root_of_unity(curve, n)``, libff's.
        ``coset`` (an int g): the coset FFT -- values[i] times g^i first.  ``inverse``: w^-1 and the scale n^-1, with
        ``coset`` also g^-j on the way out: the inverse of the two above.  ``tile_log2``: stages per global pass, 0 =
        default (``plan_fr_fft`` tells).  ``pre``, ``post``, ``scale`` (ints): the general form
        ``out[j] = post^j scale sum_i pre^i values[i] w^(i j)``, each in place of what the flags derive."""
        limbs = _fr_limbs(curve)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        n = int(values.shape[0]) if values.ndim == 2 else 0
        if n:
            assert values.shape == (n, limbs), "values must be (n, fr_limbs) uint64"
        if out is None:
            out = np.zeros((n, limbs), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (n, limbs)
        w, pre, post, scale = self._fr_params(curve, n, omega, inverse, coset, plain, (pre, post, scale))
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_fft(self.h, curve, _np_ptr(values) if n else None, ctypes.c_size_t(n), _opt_ptr(w), _opt_ptr(pre),
                                    _opt_ptr(post), _opt_ptr(scale), int(tile_log2), ctypes.byref(o), _np_ptr(out) if n else None)
        self._check(rc, "amdmsm_fr_fft")
        return out

    def fr_matrix_load(self, curve, offsets, cols, coeffs, n_cols, plain=False):
        """Keep a CSR matrix over Fr on the device (``amdmsm_fr_matrix_load``): ``offsets`` (n_rows + 1), ``cols`` (nnz),
        ``coeffs`` (nnz, fr_limbs) uint64 records -- Montgomery residues, with ``plain`` plain integers.  Returns an
        ``FrMatrix``."""
        offsets, cols, coeffs, n_rows, ptr = _csr_arrays(curve, offsets, cols, coeffs)
        h = ctypes.c_uint64(0)
        rc = self.lib.amdmsm_fr_matrix_load(self.h, curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols), ptr(offsets),
                                            ptr(cols), ptr(coeffs), int(plain), ctypes.byref(h))
        self._check(rc, "amdmsm_fr_matrix_load")
        return FrMatrix(self, h.value, curve, n_rows, int(n_cols))

    def fr_matrix_load_transposed(self, curve, offsets, cols, coeffs, n_cols, plain=False):
        """Keep the transpose of a CSR matrix M on the device (``amdmsm_fr_matrix_load_transposed``): the arguments are
        those of ``fr_matrix_load`` for M, the ``FrMatrix`` has ``n_cols`` rows and M's rows as columns --
        ``fr_matrix_apply(mat, u)[c]`` is the sum of ``coeff * u[i]`` over the entries (i, c) of M."""
        offsets, cols, coeffs, n_rows, ptr = _csr_arrays(curve, offsets, cols, coeffs)
        h = ctypes.c_uint64(0)
        rc = self.lib.amdmsm_fr_matrix_load_transposed(self.h, curve, ctypes.c_size_t(n_rows), ctypes.c_size_t(n_cols),
                                                       ptr(offsets), ptr(cols), ptr(coeffs), int(plain), ctypes.byref(h))
        self._check(rc, "amdmsm_fr_matrix_load_transposed")
        return FrMatrix(self, h.value, curve, int(n_cols), n_rows)

    def fr_matrix_apply(self, mat, x, n_out=None, plain=False):
        """``out[i] = sum_k coeffs[k] x[cols[k]]`` over row i (``amdmsm_fr_matrix_apply``): ``x`` (n_x >= n_cols, fr_limbs)
        uint64 records in the form ``plain`` says, the result -- ``n_out`` records, the rows and zeros behind them --
        in the same form."""
        x, n_x = _fr_array(mat.curve, x)
        n_out = mat.n_rows if n_out is None else int(n_out)
        out = np.zeros((n_out, x.shape[1]), dtype=np.uint64)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_matrix_apply(self.h, ctypes.c_uint64(mat.handle), _np_ptr(x) if n_x else None, ctypes.c_size_t(n_x),
                                             _np_ptr(out) if n_out else None, ctypes.c_size_t(n_out), ctypes.byref(o))
        self._check(rc, "amdmsm_fr_matrix_apply")
        return out

    def fr_matrix_apply_device(self, mat, d_x, n_x, d_out, n_out, plain=False, stream=None):
        """``fr_matrix_apply`` on device-resident vectors (``amdmsm_fr_matrix_apply_device``): enqueued on ``stream``, not
        synchronised; records n_rows .. n_out - 1 of ``d_out`` are written as zero."""
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_matrix_apply_device(self.h, ctypes.c_uint64(mat.handle),
                                                           _opt_dev(d_x), ctypes.c_size_t(n_x), _opt_dev(d_out), ctypes.c_size_t(n_out),
                                                           ctypes.byref(o)), "amdmsm_fr_matrix_apply_device")

    def group_matrix_apply(self, mat, group, points, *, base_form=multi_exp_base_form_normal, out_form=OUT_LIBFF,
                           chunk_entries=0, stride_bytes=None, out=None):
        """Sparse matrix times point vector on the handle of an Fr matrix (``amdmsm_group_matrix_apply``):
        ``out[i] = sum_k coeff[k] * points[col[k]]`` over the kept entries of row i of ``mat``, the group's zero for a row
        without any.  ``points``: (n >= mat.n_cols, 3 * coordinate limbs) libff records of ``group`` of the matrix's curve
        in ``base_form``; the result is ``mat.n_rows`` records in ``out_form``.  ``chunk_entries``: general-coefficient
        entries worked through at a time, 0 = automatic (``plan_group_matrix`` tells); the results do not depend on it.
        ``stride_bytes``: bytes between two records of ``points`` (default: packed).  ``out``: result array to fill."""
        s = sizes(mat.curve, group)
        points = np.ascontiguousarray(points, dtype=np.uint64)
        n = _records(points, stride_bytes, s["g_bytes"])
        if n and stride_bytes is None:
            assert points.shape == (n, s["g_bytes"] // 8), "points must be (n, 3*coord_limbs) uint64"
        out = _result_array(out, mat.n_rows, s["g_bytes"])
        o = self._opts(out_form=out_form)
        rc = self.lib.amdmsm_group_matrix_apply(self.h, mat.curve, group, ctypes.c_uint64(mat.handle), _np_ptr(points) if n else None,
                                                ctypes.c_size_t(s["g_bytes"] if stride_bytes is None else stride_bytes), base_form,
                                                ctypes.c_size_t(n), _np_ptr(out) if mat.n_rows else None,
                                                ctypes.c_size_t(chunk_entries), ctypes.byref(o))
        self._check(rc, "amdmsm_group_matrix_apply")
        return out

    def group_matrix_apply_device(self, mat, group, d_points_affine, n_points, d_out_xyz, *, out_form=OUT_LIBFF, chunk_entries=0,
                                  stream=None):
        """``group_matrix_apply`` on device-resident inputs (``amdmsm_group_matrix_apply_device``): ``n_points`` compact
        affine records (``import_bases_device``) in, ``mat.n_rows`` records written to ``d_out_xyz``; enqueued on
        ``stream``, not synchronised.  The chain of a phase-2 setup: ``group_fft_device`` with the inverse twiddles and
        ``fold_vec_device`` by n^-1, ``import_bases_device``, this entry, ``write_points_file``."""
        o = self._opts(out_form=out_form, stream=stream)
        self._check(self.lib.amdmsm_group_matrix_apply_device(self.h, mat.curve, group, ctypes.c_uint64(mat.handle),
                                                              _opt_dev(d_points_affine), ctypes.c_size_t(n_points),
                                                              _opt_dev(d_out_xyz), ctypes.c_size_t(chunk_entries),
                                                              ctypes.byref(o)), "amdmsm_group_matrix_apply_device")

    def plan_group_matrix(self, mat, group, chunk_entries=0):
        """What ``group_matrix_apply`` runs for the handle ``mat`` (``amdmsm_plan_group_matrix``, read-only): entries kept
        by kind, wave jobs, partial sums, chunks for this ``chunk_entries``, workspace bytes and launches."""
        out = (ctypes.c_size_t * 8)()
        self._check(self.lib.amdmsm_plan_group_matrix(self.h, mat.curve, group, ctypes.c_uint64(mat.handle),
                                                      ctypes.c_size_t(chunk_entries), out), "amdmsm_plan_group_matrix")
        return {"general": out[0], "plus_minus_one": out[1], "wave_jobs": out[2], "partials": out[3], "chunks": out[4],
                "workspace_bytes": out[5], "launches": out[6]}

    def _scan_flags(self, reverse, exclusive):
        return (SCAN_REVERSE if reverse else 0) | (SCAN_EXCLUSIVE if exclusive else 0)

    def fr_scan(self, curve, a=None, b=None, *, a_const=None, init=None, reverse=False, exclusive=False, plain=False,
                tile_log2=0, flags=None):
        """The recurrence ``y_i = a_i y_(i-1) + b_i`` over host arrays (``amdmsm_fr_scan``): ``a`` / ``b`` (n, fr_limbs)
        uint64 records or None, ``a_const`` / ``init`` ints (or records as arrays).  ``reverse``: from the last record
        down; ``exclusive``: ``out[i]`` is the value that enters record i.  Returns ``(out, total)``, total a record."""
        limbs, r = _fr_limbs(curve), fr_modulus(curve, G1)
        (a, n_a), (b, n_b) = _fr_array(curve, a), _fr_array(curve, b)
        n = n_b if a is None else n_a
        assert a is None or b is None or a.shape == b.shape, "a and b: one record each per position"
        out, total = np.zeros((n, limbs), dtype=np.uint64), np.zeros(limbs, dtype=np.uint64)
        ac, ini = _fr_host_record(a_const, limbs, r, plain), _fr_host_record(init, limbs, r, plain)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_scan(self.h, curve, ctypes.c_size_t(n), _opt_ptr(a), _opt_ptr(ac), _opt_ptr(b), _opt_ptr(ini),
                                     self._scan_flags(reverse, exclusive) if flags is None else int(flags), int(tile_log2),
                                     ctypes.byref(o), _np_ptr(out), _np_ptr(total))
        self._check(rc, "amdmsm_fr_scan")
        return out, total

    def fr_scan_device(self, curve, n, d_out, d_a=None, d_b=None, *, a_const=None, init=None, d_total=None, reverse=False,
                       exclusive=False, plain=False, tile_log2=0, stream=None, flags=None):
        """``fr_scan`` on ``n`` device-resident records (``amdmsm_fr_scan_device``); ``d_out`` may be ``d_a`` or ``d_b``,
        ``d_total`` (one record) may be None; enqueued on ``stream``, not synchronised."""
        limbs, r = _fr_limbs(curve), fr_modulus(curve, G1)
        ac, ini = _fr_host_record(a_const, limbs, r, plain), _fr_host_record(init, limbs, r, plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        ptr, dev = _opt_ptr, _opt_dev
        self._check(self.lib.amdmsm_fr_scan_device(self.h, curve, ctypes.c_size_t(n), dev(d_a), ptr(ac), dev(d_b), ptr(ini),
                                                   self._scan_flags(reverse, exclusive) if flags is None else int(flags),
                                                   int(tile_log2), ctypes.byref(o), dev(d_out), dev(d_total)),
                    "amdmsm_fr_scan_device")

    def fr_batch_invert(self, curve, values, plain=False):
        """``out[i] = 1 / values[i]``, 0 where ``values[i]`` is 0 (``amdmsm_fr_batch_invert``): (n, fr_limbs) uint64
        records in the form ``plain`` says.  Returns ``(out, zero_count)``."""
        values, n = _fr_array(curve, values)
        out, zeros = np.zeros_like(values), ctypes.c_uint64(0)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_batch_invert(self.h, curve, ctypes.c_size_t(n), _np_ptr(values) if n else None, ctypes.byref(o),
                                             _np_ptr(out) if n else None, ctypes.byref(zeros))
        self._check(rc, "amdmsm_fr_batch_invert")
        return out, int(zeros.value)

    def fr_batch_invert_device(self, curve, n, d_values, d_out, d_zero_count=None, plain=False, tile_log2=0, stream=None):
        """``fr_batch_invert`` on ``n`` device-resident records (``amdmsm_fr_batch_invert_device``); ``d_out`` may be
        ``d_values``; ``d_zero_count``: a uint64 in device memory or None; enqueued on ``stream``, not synchronised."""
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_batch_invert_device(self.h, curve, ctypes.c_size_t(n), _opt_dev(d_values), int(tile_log2),
                                                           ctypes.byref(o), _opt_dev(d_out), _opt_dev(d_zero_count)),
                    "amdmsm_fr_batch_invert_device")

    def _coset_record(self, curve, coset, plain):
        return None if coset is None else _fr_record(coset, _fr_limbs(curve), fr_modulus(curve, G1), plain)

    def fr_domain_fft(self, curve, values, inverse=False, coset=None, plain=False, tile_log2=0, out=None):
        """The transform over libfqfft's evaluation domain of ``len(values)`` points (``amdmsm_fr_domain_fft``;
        ``fr_domain`` tells which sizes are domain sizes): ``out[j] = A(g x_j)`` for the polynomial with the coefficients
        ``values``, or with ``inverse`` the coefficients from the values.  ``coset`` (an int g): the shift, None = 1.
        Records and ``tile_log2`` as for ``fr_fft``."""
        values, m = _fr_array(curve, values)
        limbs = _fr_limbs(curve)
        if out is None:
            out = np.zeros((m, limbs), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (m, limbs)
        g = self._coset_record(curve, coset, plain)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_domain_fft(self.h, curve, _opt_ptr(values), ctypes.c_size_t(m), DOMAIN_INVERSE if inverse else 0,
                                           _opt_ptr(g), int(tile_log2), ctypes.byref(o), _np_ptr(out))
        self._check(rc, "amdmsm_fr_domain_fft")
        return out

    def fr_domain_fft_device(self, curve, d_values, m, d_out, inverse=False, coset=None, plain=False, tile_log2=0, stream=None):
        """``fr_domain_fft`` on ``m`` device-resident records; ``d_out`` may be ``d_values``; enqueued on ``stream``, not
        synchronised."""
        g = self._coset_record(curve, coset, plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_domain_fft_device(self.h, curve, _opt_dev(d_values), ctypes.c_size_t(m),
                                                         DOMAIN_INVERSE if inverse else 0, _opt_ptr(g), int(tile_log2),
                                                         ctypes.byref(o), _opt_dev(d_out)), "amdmsm_fr_domain_fft_device")

    def fr_domain_fft_batch_device(self, curve, d_values, m, batch, d_out, in_stride=None, out_stride=None, inverse=False,
                                   coset=None, plain=False, tile_log2=0, stream=None):
        """``fr_domain_fft_device`` over ``batch`` vectors of ``m`` records (``amdmsm_fr_domain_fft_batch_device``), vector
        v at ``v * in_stride`` / ``v * out_stride`` records (None = m: packed); every vector gets what the single call
        gives it."""
        g = self._coset_record(curve, coset, plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_domain_fft_batch_device(
            self.h, curve, _opt_dev(d_values), ctypes.c_size_t(m), ctypes.c_size_t(batch),
            ctypes.c_size_t(m if in_stride is None else in_stride), ctypes.c_size_t(m if out_stride is None else out_stride),
            DOMAIN_INVERSE if inverse else 0, _opt_ptr(g), int(tile_log2), ctypes.byref(o), _opt_dev(d_out)),
            "amdmsm_fr_domain_fft_batch_device")

    def fr_fft_batch(self, curve, values, omega=None, inverse=False, coset=None, plain=False, tile_log2=0, out=None, *,
                     pre=None, post=None, scale=None):
        """``fr_fft`` of every row of ``values``, a (batch, n, fr_limbs) uint64 array, with one set of parameters
        (``amdmsm_fr_fft_batch``): one chain of passes whose grid covers the whole batch.  Returns an array of the same
        shape; row v is what ``fr_fft(values[v], ...)`` gives, bit for bit."""
        limbs = _fr_limbs(curve)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        assert values.ndim == 3 and values.shape[2] == limbs, "values must be (batch, n, fr_limbs) uint64"
        batch, n = int(values.shape[0]), int(values.shape[1])
        if out is None:
            out = np.zeros((batch, n, limbs), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (batch, n, limbs)
        w, pre, post, scale = self._fr_params(curve, n, omega, inverse, coset, plain, (pre, post, scale))
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_fft_batch(self.h, curve, _np_ptr(values) if values.size else None, ctypes.c_size_t(n),
                                          ctypes.c_size_t(batch), _opt_ptr(w), _opt_ptr(pre), _opt_ptr(post), _opt_ptr(scale),
                                          int(tile_log2), ctypes.byref(o), _np_ptr(out) if out.size else None)
        self._check(rc, "amdmsm_fr_fft_batch")
        return out

    def fr_fft_batch_device(self, curve, d_values, n, batch, d_out, in_stride=None, out_stride=None, omega=None, inverse=False,
                            coset=None, plain=False, tile_log2=0, stream=None, *, pre=None, post=None, scale=None):
        """``fr_fft_batch`` on device-resident records (``amdmsm_fr_fft_batch_device``): vector v starts ``v * in_stride``
        records into ``d_values`` and ``v * out_stride`` records into ``d_out`` (None = n: packed); ``d_out`` may be
        ``d_values`` with equal strides; enqueued on ``stream``, not synchronised."""
        w, pre, post, scale = self._fr_params(curve, n, omega, inverse, coset, plain, (pre, post, scale))
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_fft_batch_device(
            self.h, curve, _opt_dev(d_values), ctypes.c_size_t(n), ctypes.c_size_t(batch),
            ctypes.c_size_t(n if in_stride is None else in_stride), ctypes.c_size_t(n if out_stride is None else out_stride),
            _opt_ptr(w), _opt_ptr(pre), _opt_ptr(post), _opt_ptr(scale), int(tile_log2), ctypes.byref(o), _opt_dev(d_out)),
            "amdmsm_fr_fft_batch_device")

    def _blind_records(self, curve, blind, plain):
        if blind is None:
            return None
        assert len(blind) == 3, "blind: d1, d2, d3"
        limbs, r = _fr_limbs(curve), fr_modulus(curve, G1)
        return np.array([_fr_record(x, limbs, r, plain) for x in blind], dtype=np.uint64).reshape(3, limbs)

    def qap_witness_map(self, curve, mat_a, mat_b, mat_c, z, m, blind=None, plain=False):
        """libsnark's ``r1cs_to_qap_witness_map`` as one call (``amdmsm_fr_qap_witness_map``): the ``m + 1`` coefficients of
        H with ``(A + d1 Z)(B + d2 Z) - (C + d3 Z) = H Z`` on the domain of ``m`` points (a size ``fr_domain`` answers
        with), A, B, C interpolating the applies of the three ``FrMatrix`` handles on ``z`` (an (n_z, fr_limbs) uint64
        array), zero-filled to m.  ``blind``: the ints (d1, d2, d3), None for none.  Records in the form ``plain`` says."""
        z, n_z = _fr_array(curve, z)
        h = np.zeros((m + 1, _fr_limbs(curve)), dtype=np.uint64)
        b = self._blind_records(curve, blind, plain)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_qap_witness_map(self.h, curve, ctypes.c_uint64(mat_a.handle), ctypes.c_uint64(mat_b.handle),
                                                ctypes.c_uint64(mat_c.handle), _np_ptr(z) if n_z else None, ctypes.c_size_t(n_z),
                                                ctypes.c_size_t(m), _opt_ptr(b), ctypes.byref(o), _np_ptr(h))
        self._check(rc, "amdmsm_fr_qap_witness_map")
        return h

    def qap_witness_map_device(self, curve, mat_a, mat_b, mat_c, d_z, n_z, m, d_h, blind=None, plain=False, stream=None):
        """``qap_witness_map`` from ``n_z`` device-resident records into the ``m + 1`` records of ``d_h``
        (``amdmsm_fr_qap_witness_map_device``); enqueued on ``stream``, not synchronised."""
        b = self._blind_records(curve, blind, plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_qap_witness_map_device(
            self.h, curve, ctypes.c_uint64(mat_a.handle), ctypes.c_uint64(mat_b.handle), ctypes.c_uint64(mat_c.handle),
            _opt_dev(d_z), ctypes.c_size_t(n_z), ctypes.c_size_t(m), _opt_ptr(b), ctypes.byref(o), _opt_dev(d_h)),
            "amdmsm_fr_qap_witness_map_device")

    def fr_domain_divide_by_z(self, curve, values, coset, plain=False, out=None):
        """``out[j] = values[j] / Z(g x_j)`` over the domain of ``len(values)`` points (``amdmsm_fr_domain_divide_by_z``),
        g = ``coset`` (an int); refused where Z has a zero on the coset."""
        values, m = _fr_array(curve, values)
        limbs = _fr_limbs(curve)
        if out is None:
            out = np.zeros((m, limbs), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == (m, limbs)
        g = self._coset_record(curve, coset, plain)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_domain_divide_by_z(self.h, curve, ctypes.c_size_t(m), _opt_ptr(values), _opt_ptr(g), ctypes.byref(o),
                                                   _np_ptr(out))
        self._check(rc, "amdmsm_fr_domain_divide_by_z")
        return out

    def fr_domain_divide_by_z_device(self, curve, m, d_values, d_out, coset, plain=False, stream=None):
        """``fr_domain_divide_by_z`` on ``m`` device-resident records; ``d_out`` may be ``d_values``; enqueued on
        ``stream``, not synchronised."""
        g = self._coset_record(curve, coset, plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_domain_divide_by_z_device(self.h, curve, ctypes.c_size_t(m), _opt_dev(d_values), _opt_ptr(g),
                                                                 ctypes.byref(o), _opt_dev(d_out)),
                    "amdmsm_fr_domain_divide_by_z_device")

    def fr_domain_lagrange(self, curve, m, t, plain=False):
        """The Lagrange vector of the domain of ``m`` points at ``t`` (an int; ``amdmsm_fr_domain_lagrange``):
        ``out[j] = L_j(t)``, (m, fr_limbs) uint64 records in the form ``plain`` says -- libfqfft's
        ``evaluate_all_lagrange_polynomials(t)``; the unit vector where ``t`` is a point of the domain."""
        limbs = _fr_limbs(curve)
        out = np.zeros((m, limbs), dtype=np.uint64)
        tt = _fr_host_record(t, limbs, fr_modulus(curve, G1), plain)
        o = self._opts(scalars_plain=plain)
        rc = self.lib.amdmsm_fr_domain_lagrange(self.h, curve, ctypes.c_size_t(m), _opt_ptr(tt), ctypes.byref(o), _np_ptr(out))
        self._check(rc, "amdmsm_fr_domain_lagrange")
        return out

    def fr_domain_lagrange_device(self, curve, m, t, d_out, plain=False, stream=None):
        """``fr_domain_lagrange`` into ``m`` device-resident records (``amdmsm_fr_domain_lagrange_device``); enqueued on
        ``stream``, not synchronised."""
        tt = _fr_host_record(t, _fr_limbs(curve), fr_modulus(curve, G1), plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_domain_lagrange_device(self.h, curve, ctypes.c_size_t(m), _opt_ptr(tt), ctypes.byref(o),
                                                              _opt_dev(d_out)), "amdmsm_fr_domain_lagrange_device")

    def fr_lincomb_device(self, curve, n, d_vectors, scalars, d_out, plain=False, stream=None):
        """``d_out[i] = sum_j scalars[j] * d_vectors[j][i]`` over ``n`` device-resident records
        (``amdmsm_fr_lincomb_device``): 1 to 4 device pointers, as many ``scalars`` (ints, or a (k, fr_limbs) uint64 array
        taken as it stands); ``d_out`` may be one of the vectors; enqueued on ``stream``, not synchronised."""
        limbs, r = _fr_limbs(curve), fr_modulus(curve, G1)
        k = len(d_vectors)
        if isinstance(scalars, np.ndarray):
            s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, limbs)
        else:
            s = np.array([_fr_record(x, limbs, r, plain) for x in scalars], dtype=np.uint64).reshape(-1, limbs)
        assert s.shape[0] == k, "one scalar per vector"
        ptrs = (ctypes.c_void_p * max(k, 1))(*[_opt_dev(x) for x in d_vectors])
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_lincomb_device(self.h, curve, ctypes.c_size_t(n), k, ptrs, _np_ptr(s) if s.size else None,
                                                      ctypes.byref(o), _opt_dev(d_out)), "amdmsm_fr_lincomb_device")

    def batch_exp_timings(self):
        """device times (ms) of the last batch_exp: inputs H2D, window table (0 = reused), exponentiations, results D2H.
        After ``batch_exp_device`` the call is waited for; ``h2d_ms`` is then the upload of g / coeff and ``d2h_ms`` the
        normalisation (0 for ``OUT_LIBFF``)."""
        ms = (ctypes.c_float * 4)()
        self._check(self.lib.amdmsm_get_batch_exp_timings(self.h, ms), "amdmsm_get_batch_exp_timings")
        return {"h2d_ms": ms[0], "table_ms": ms[1], "exp_ms": ms[2], "d2h_ms": ms[3]}

    def sum_points(self, curve, group, points_jacobian, out_form=OUT_AFFINE):
        """Sum of engine-Jacobian partial results (the serial tail of multiexp.tcc:681-687)."""
        pts = np.ascontiguousarray(points_jacobian, dtype=np.uint64)
        s = sizes(curve, group)
        k = pts.shape[0]
        d_pts, d_out = self.malloc(max(1, pts.nbytes)), self.malloc(s["g_bytes"])
        try:
            if k:
                self.h2d(d_pts, pts)
            rc = self.lib.amdmsm_sum_points_device(self.h, curve, group, d_pts, k, out_form, d_out, None)
            self._check(rc, "amdmsm_sum_points_device")
            out = np.zeros(s["g_bytes"] // 8, dtype=np.uint64)
            self.d2h(out, d_out)
            return out
        finally:
            self.free(d_pts)
            self.free(d_out)

    # -------------------------------------------------------- raw device API
    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self.lib.amdmsm_malloc(self.h, ctypes.c_size_t(nbytes), ctypes.byref(p)), "amdmsm_malloc")
        return p

    def free(self, p):
        self._check(self.lib.amdmsm_free(self.h, p), "amdmsm_free")

    def h2d(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.amdmsm_memcpy_h2d(self.h, d_ptr, _np_ptr(arr), ctypes.c_size_t(arr.nbytes)), "h2d")

    def d2h(self, arr, d_ptr):
        assert arr.flags["C_CONTIGUOUS"]
        self._check(self.lib.amdmsm_memcpy_d2h(self.h, _np_ptr(arr), d_ptr, ctypes.c_size_t(arr.nbytes)), "d2h")

    def synchronize(self):
        self._check(self.lib.amdmsm_synchronize(self.h), "amdmsm_synchronize")

    def import_bases_device(self, curve, group, d_src_xyz, stride_bytes, base_form, n, d_dst_affine, stream=None):
        self._check(self.lib.amdmsm_import_bases_device(self.h, curve, group, _vp(d_src_xyz),
                                                        ctypes.c_size_t(stride_bytes), base_form,
                                                        ctypes.c_size_t(n), _vp(d_dst_affine),
                                                        _vp(stream)), "amdmsm_import_bases_device")

    def export_affine_device(self, curve, group, d_src_affine, n, d_dst_xyz, stream=None):
        self._check(self.lib.amdmsm_export_affine_device(self.h, curve, group, _vp(d_src_affine),
                                                         ctypes.c_size_t(n), _vp(d_dst_xyz),
                                                         _vp(stream)), "amdmsm_export_affine_device")

    def msm_device(self, curve, group, d_bases_affine, d_scalars, n, d_out_xyz, out_form=OUT_LIBFF,
                   window_bits=0, segment_len=0, scalars_plain=False, stream=None):
        o = self._opts(window_bits, segment_len, out_form, scalars_plain, stream)
        self._check(self.lib.amdmsm_msm_device(self.h, curve, group, _vp(d_bases_affine),
                                               _vp(d_scalars), ctypes.c_size_t(n),
                                               _vp(d_out_xyz), ctypes.byref(o)), "amdmsm_msm_device")

    def msm_device_short(self, curve, group, d_bases_affine, d_scalars, kind, n, d_out_xyz, bits=0, out_form=OUT_LIBFF,
                         window_bits=0, segment_len=0, scalars_plain=False, stream=None):
        """``msm_device`` on scalars of ``kind`` (``SCALAR_*``) known to be short; asynchronous only with ``bits=0``."""
        o = self._opts(window_bits, segment_len, out_form, scalars_plain, stream)
        d = scalar_desc(kind, bits)
        self._check(self.lib.amdmsm_msm_device_short(self.h, curve, group, _vp(d_bases_affine), _vp(d_scalars),
                                                     ctypes.byref(d), ctypes.c_size_t(n), _vp(d_out_xyz),
                                                     ctypes.byref(o)), "amdmsm_msm_device_short")

    def scalar_bits(self, curve, group, d_scalars, kind, n, scalars_plain=False):
        """Bit length of the longest of ``n`` device-resident scalars of ``kind`` (0: all zero); synchronises."""
        d = scalar_desc(kind, 0)
        bits = ctypes.c_int(0)
        self._check(self.lib.amdmsm_scalar_bits_device(self.h, curve, group, _vp(d_scalars), ctypes.c_size_t(n),
                                                       ctypes.byref(d), int(scalars_plain), ctypes.byref(bits)),
                    "amdmsm_scalar_bits_device")
        return bits.value

    def msm_device_batch(self, curve, group, d_bases_affine, d_scalars, n, d_out_xyz, out_form=OUT_LIBFF,
                         window_bits=0, scalars_plain=False, stream=None):
        """amdmsm_msm_device_batch: len(d_bases_affine) MSMs of n points each (lists of device pointers) in one call;
        the tails of all of them run as one set of kernels."""
        k = len(d_bases_affine)
        pb = (ctypes.c_void_p * k)(*[_vp(x) for x in d_bases_affine])
        ps = (ctypes.c_void_p * k)(*[_vp(x) for x in d_scalars])
        po = (ctypes.c_void_p * k)(*[_vp(x) for x in d_out_xyz])
        o = self._opts(window_bits, 0, out_form, scalars_plain, stream)
        self._check(self.lib.amdmsm_msm_device_batch(self.h, curve, group, k, pb, ps, ctypes.c_size_t(n), po, ctypes.byref(o)),
                    "amdmsm_msm_device_batch")

    def msm_device_batch_items(self, curve, group, items, d_shared_scalars=None, shared_n=0, out_form=OUT_LIBFF,
                               window_bits=0, scalars_plain=False, stream=None):
        """amdmsm_msm_device_batch_items: ``items`` are dicts of device pointers -- ``bases`` (compact affine), ``n``,
        ``out`` and one of ``scalars`` / ``offset`` / ``index`` (a device array of n uint32).  A call with index lists
        synchronises to learn whether an index was out of range (AmdMsmError)."""
        k = len(items)
        arr = (BatchItemStruct * max(k, 1))()
        for j, it in enumerate(items):
            arr[j] = BatchItemStruct(ctypes.sizeof(BatchItemStruct), _vp(it["bases"]) if it.get("bases") else None, int(it["n"]),
                                     _vp(it["scalars"]) if it.get("scalars") else None, int(it.get("offset", 0)),
                                     _vp(it["index"]) if it.get("index") else None, _vp(it["out"]))
        o = self._opts(window_bits, 0, out_form, scalars_plain, stream)
        self._check(self.lib.amdmsm_msm_device_batch_items(self.h, curve, group, k, arr,
                                                           _vp(d_shared_scalars) if d_shared_scalars else None,
                                                           ctypes.c_size_t(shared_n), ctypes.byref(o)),
                    "amdmsm_msm_device_batch_items")

    def scalar_mul_vec_device(self, curve, group, d_points_affine, d_scalars, n, d_out_xyz, out_form=OUT_LIBFF,
                              scalars_plain=False, chunk_points=0, stream=None):
        """``scalar_mul_vec`` on device-resident compact affine points; enqueued on ``stream``, not synchronised."""
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain, stream=stream)
        self._check(self.lib.amdmsm_scalar_mul_vec_device(self.h, curve, group, _vp(d_points_affine), _vp(d_scalars),
                                                          ctypes.c_size_t(n), _vp(d_out_xyz), ctypes.c_size_t(chunk_points),
                                                          ctypes.byref(o)), "amdmsm_scalar_mul_vec_device")

    def fold_vec_device(self, curve, group, d_points_list, scalars, n, d_out_xyz, out_form=OUT_LIBFF, scalars_plain=False,
                        chunk_points=0, stream=None):
        """``fold_vec`` on device-resident compact affine vectors (a list of device pointers; ``scalars`` stays a host
        array of k records); enqueued on ``stream``, not synchronised.  Rounds chain on the device: ``OUT_AFFINE``, then
        ``import_bases_device(d_out_xyz, ..., multi_exp_base_form_special, ...)`` gives the next round's vector."""
        k = len(d_points_list)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[_vp(x) for x in d_points_list])
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain, stream=stream)
        self._check(self.lib.amdmsm_fold_vec_device(self.h, curve, group, k, ptrs, _np_ptr(scalars) if scalars.size else None,
                                                    ctypes.c_size_t(n), _vp(d_out_xyz), ctypes.c_size_t(chunk_points),
                                                    ctypes.byref(o)), "amdmsm_fold_vec_device")

    def group_fft_device(self, curve, group, d_points, n, d_twiddles, d_out_xyz, out_form=OUT_LIBFF, scalars_plain=False,
                         chunk_points=0, stream=None):
        """``group_fft`` on device-resident inputs: ``n`` compact affine points, ``n / 2`` twiddles (None will do for
        n <= 2), ``n`` records written to ``d_out_xyz``; enqueued on ``stream``, not synchronised.  The inverse chains on
        the device: ``OUT_AFFINE``, ``import_bases_device(d_out_xyz, ..., multi_exp_base_form_special, ...)``, then
        ``fold_vec_device`` with k = 1 and the scalar n^-1."""
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain, stream=stream)
        self._check(self.lib.amdmsm_group_fft_device(self.h, curve, group, None if d_points is None else _vp(d_points),
                                                     ctypes.c_size_t(n), None if d_twiddles is None else _vp(d_twiddles),
                                                     None if d_out_xyz is None else _vp(d_out_xyz),
                                                     ctypes.c_size_t(chunk_points), ctypes.byref(o)), "amdmsm_group_fft_device")

    def fr_fft_device(self, curve, d_values, n, d_out, omega=None, inverse=False, coset=None, plain=False, tile_log2=0,
                      stream=None, *, pre=None, post=None, scale=None):
        """``fr_fft`` on ``n`` device-resident records; ``d_out`` may be ``d_values`` (in place); enqueued on ``stream``,
        not synchronised."""
        w, pre, post, scale = self._fr_params(curve, n, omega, inverse, coset, plain, (pre, post, scale))
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_fft_device(self.h, curve, _opt_dev(d_values), ctypes.c_size_t(n), _opt_ptr(w), _opt_ptr(pre),
                                                  _opt_ptr(post), _opt_ptr(scale), int(tile_log2), ctypes.byref(o), _opt_dev(d_out)),
                    "amdmsm_fr_fft_device")

    def fr_powers_device(self, curve, base, n, d_out, plain=False, stream=None):
        """``d_out[i] = base^i`` for i < n (``amdmsm_fr_powers_device``; ``base`` an int): twiddles for
        ``group_fft_device``, coset powers for ``scalar_mul_vec_device``; enqueued on ``stream``, not synchronised."""
        b = _fr_record(base, _fr_limbs(curve), fr_modulus(curve, G1), plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_powers_device(self.h, curve, _np_ptr(b), ctypes.c_size_t(n), ctypes.byref(o), _opt_dev(d_out)),
                    "amdmsm_fr_powers_device")

    def fr_muladd_device(self, curve, n, d_a, d_b, d_out, d_c=None, k=None, plain=False, stream=None):
        """``d_out[i] = (a_i * b_i - c_i) * k`` (``amdmsm_fr_muladd_device``; ``d_c`` None = 0, ``k`` an int, None = 1);
        ``d_out`` may be any input; enqueued on ``stream``, not synchronised."""
        kk = None if k is None else _fr_record(k, _fr_limbs(curve), fr_modulus(curve, G1), plain)
        o = self._opts(scalars_plain=plain, stream=stream)
        self._check(self.lib.amdmsm_fr_muladd_device(self.h, curve, ctypes.c_size_t(n), _vp(d_a), _vp(d_b), _opt_dev(d_c),
                                                     _opt_ptr(kk), ctypes.byref(o), _vp(d_out)), "amdmsm_fr_muladd_device")

    def msm_device_segments(self, curve, group, d_bases_affine, n_bases, d_scalars, n_terms, offsets, d_out, *,
                            shared_bases=False, long_from=0, out_form=OUT_LIBFF, scalars_plain=False, chunk_terms=0,
                            stream=None):
        """``multi_exp_segments`` on device-resident compact affine bases and scalars (``offsets`` stays a host array);
        ``len(offsets) - 1`` records are written to ``d_out``; enqueued on ``stream``, not synchronised."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        m = max(int(offs.shape[0]) - 1, 0)
        o = self._opts(out_form=out_form, scalars_plain=scalars_plain, stream=stream)
        self._check(self.lib.amdmsm_set_segments_chunk_terms(self.h, ctypes.c_size_t(chunk_terms)),
                    "amdmsm_set_segments_chunk_terms")
        try:
            rc = self.lib.amdmsm_msm_device_segments(
                self.h, curve, group, _vp(d_bases_affine), ctypes.c_size_t(n_bases), _vp(d_scalars), ctypes.c_size_t(n_terms),
                _np_ptr(offs) if offs.shape[0] else None, ctypes.c_size_t(m),
                ctypes.c_uint(SEG_SHARED_BASES if shared_bases else 0), ctypes.c_size_t(long_from), _vp(d_out),
                ctypes.byref(o))
        finally:
            self.lib.amdmsm_set_segments_chunk_terms(self.h, ctypes.c_size_t(0))
        self._check(rc, "amdmsm_msm_device_segments")

    def precompute_bases_device(self, curve, group, d_bases_affine, n, c, num_digits, d_table, stream=None):
        self._check(self.lib.amdmsm_precompute_bases_device(
            self.h, curve, group, _vp(d_bases_affine), ctypes.c_size_t(n), ctypes.c_size_t(c),
            ctypes.c_size_t(num_digits), _vp(d_table), _vp(stream)),
            "amdmsm_precompute_bases_device")

    def msm_precomputed_device(self, curve, group, d_table, d_scalars, n, c, num_digits, d_out_xyz,
                               out_form=OUT_LIBFF, segment_len=0, scalars_plain=False, stream=None):
        o = self._opts(0, segment_len, out_form, scalars_plain, stream)
        self._check(self.lib.amdmsm_msm_precomputed_device(
            self.h, curve, group, _vp(d_table), _vp(d_scalars), ctypes.c_size_t(n),
            ctypes.c_size_t(c), ctypes.c_size_t(num_digits), _vp(d_out_xyz), ctypes.byref(o)),
            "amdmsm_msm_precomputed_device")

    def sum_points_device(self, curve, group, d_points, k, out_form, d_out, stream=None):
        self._check(self.lib.amdmsm_sum_points_device(self.h, curve, group, _vp(d_points), k, out_form,
                                                      _vp(d_out), _vp(stream)),
                    "amdmsm_sum_points_device")

    def gen_bases_seq_device(self, curve, group, first, n, d_dst_affine, stream=None):
        self._check(self.lib.amdmsm_gen_bases_seq_device(self.h, curve, group, ctypes.c_uint64(first),
                                                         ctypes.c_size_t(n), _vp(d_dst_affine),
                                                         _vp(stream)), "amdmsm_gen_bases_seq_device")

    def set_timing(self, enable=True):
        self._check(self.lib.amdmsm_set_timing(self.h, int(enable)), "amdmsm_set_timing")

    def set_pipeline_depth(self, depth):
        """Number of MSMs that may be in flight (workspace slots, 1..4); see include/amdmsm.h."""
        self._check(self.lib.amdmsm_set_pipeline_depth(self.h, int(depth)), "amdmsm_set_pipeline_depth")

    def last_slot(self):
        return int(self.lib.amdmsm_last_slot(self.h))

    def last_timing_ticket(self):
        """ticket of the most recent timed MSM (see amdmsm_get_timings_by_ticket); -1 if none"""
        return int(self.lib.amdmsm_last_timing_ticket(self.h))

    def get_timings(self, slot=None, ticket=None):
        ms = (ctypes.c_float * MAX_PHASES)()
        if ticket is not None:
            self._check(self.lib.amdmsm_get_timings_by_ticket(self.h, ctypes.c_longlong(ticket), ms),
                        "amdmsm_get_timings_by_ticket")
        elif slot is None:
            self._check(self.lib.amdmsm_get_timings(self.h, ms), "amdmsm_get_timings")
        else:
            self._check(self.lib.amdmsm_get_slot_timings(self.h, int(slot), ms), "amdmsm_get_slot_timings")
        return {"count_ms": ms[PH_COUNT], "scatter_ms": ms[PH_SCATTER], "accumulate_ms": ms[PH_ACCUM],
                "reduce_ms": ms[PH_REDUCE], "final_ms": ms[PH_FINAL], "total_ms": ms[PH_TOTAL]}

    # ------------------------------------------------------------ test hooks
    def _dev_arrays(self, *arrs):
        ptrs = []
        for a in arrs:
            if a is None:
                ptrs.append(None)
                continue
            p = self.malloc(max(16, a.nbytes))
            self.h2d(p, a)
            ptrs.append(p)
        return ptrs

    def field_op(self, curve, group, op, a, b=None):
        """coordinate-field op over arrays: 0 mul 1 sqr 2 add 3 sub 4 neg 5 inverse"""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
        out = np.zeros_like(a)
        pa, pb, po = self._dev_arrays(a, b, out)
        try:
            self._check(self.lib.amdmsm_field_op_device(self.h, curve, group, op, pa, pb, po,
                                                        ctypes.c_size_t(a.shape[0])), "amdmsm_field_op_device")
            self.d2h(out, po)
        finally:
            for p in (pa, pb, po):
                if p is not None:
                    self.free(p)
        return out

    def field_probe(self, curve, group, impl, op, a, b=None, c=None, d=None):
        """one coordinate-field function per element (op: include/amdmsm.h amdmsm_field_probe_device) on the cold
        (impl 0) or the fully inlined (impl 1) element type; operands and result as stored words.  Returns (out, flag)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        rest = [np.ascontiguousarray(x, dtype=np.uint64) if x is not None else None for x in (b, c, d)]
        if any(x is not None and x.shape != a.shape for x in rest):
            raise ValueError("operand arrays must have one shape")
        out = np.zeros_like(a)
        flag = np.zeros(a.shape[0], dtype=np.uint32)
        ptrs = self._dev_arrays(a, *rest, out, flag)
        try:
            self._check(self.lib.amdmsm_field_probe_device(self.h, curve, group, int(impl), int(op), *ptrs,
                                                           ctypes.c_size_t(a.shape[0])), "amdmsm_field_probe_device")
            self.d2h(out, ptrs[4])
            self.d2h(flag, ptrs[5])
        finally:
            for p in ptrs:
                if p is not None:
                    self.free(p)
        return out, flag

    def xyzz_probe(self, curve, group, impl, op, acc, pt=None):
        """one extended-Jacobian function per lane (op: include/amdmsm.h amdmsm_xyzz_probe_device); acc and the
        result are (n, 4 * coordinate words) arrays of (X, Y, ZZ, ZZZ) as stored words"""
        acc = np.ascontiguousarray(acc, dtype=np.uint64)
        pt = np.ascontiguousarray(pt, dtype=np.uint64) if pt is not None else None
        if pt is not None and pt.shape[0] != acc.shape[0]:
            raise ValueError("operand arrays must have one length")
        out = np.zeros_like(acc)
        ptrs = self._dev_arrays(acc, pt, out)
        try:
            self._check(self.lib.amdmsm_xyzz_probe_device(self.h, curve, group, int(impl), int(op), *ptrs,
                                                          ctypes.c_size_t(acc.shape[0])), "amdmsm_xyzz_probe_device")
            self.d2h(out, ptrs[2])
        finally:
            for p in ptrs:
                if p is not None:
                    self.free(p)
        return out

    def rr_probe(self, curve, group, op, limbs, words_per_row, a=None, b=None, c=None, d=None, w=None, k=0, rows_per_element=1):
        """one reduced-radix function per element on raw limbs (op: include/amdmsm.h amdmsm_rr_probe_device).  a .. d:
        (rows, limbs) int32 arrays, w: (rows, words_per_row) uint32, one row per Fq component (rows_per_element = 2 for
        the Fq2 groups).  Returns (out limbs, out words, flag per element)."""
        a, b, c, d = (None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (a, b, c, d))
        w = None if w is None else np.ascontiguousarray(w, dtype=np.uint32)
        given = [x for x in (a, b, c, d, w) if x is not None]
        if not given:
            raise ValueError("no operand array: the ops without an input (the constants) still take a, rows of zero limbs, for the count")
        rows = given[0].shape[0]
        if any(x.shape[0] != rows for x in given) or rows % rows_per_element:
            raise ValueError("operand arrays must have one length, a multiple of rows_per_element")
        if any(x is not None and x.shape != (rows, limbs) for x in (a, b, c, d)) or (w is not None and w.shape != (rows, words_per_row)):
            raise ValueError("operand rows of the wrong width")
        out = np.zeros((rows, limbs), dtype=np.int32)
        outw = np.zeros((rows, words_per_row), dtype=np.uint32)
        flag = np.zeros(rows // rows_per_element, dtype=np.uint32)
        ptrs = self._dev_arrays(a, b, c, d, w, out, outw, flag)
        try:
            self._check(self.lib.amdmsm_rr_probe_device(self.h, curve, group, int(op), int(k), *ptrs,
                                                        ctypes.c_size_t(rows // rows_per_element)), "amdmsm_rr_probe_device")
            self.d2h(out, ptrs[5])
            self.d2h(outw, ptrs[6])
            self.d2h(flag, ptrs[7])
        finally:
            for p in ptrs:
                if p is not None:
                    self.free(p)
        return out, outw, flag

    def xyzz_rr_probe(self, curve, group, op, words_per_row, acc, sec=None, pt=None, fin=None, rows_per_element=1):
        """one step of one reduced-radix point function per element (op: include/amdmsm.h amdmsm_xyzz_rr_probe_device).
        acc, sec: (rows, 4 * limbs) int32; pt: (rows, 2 * words_per_row) uint32; fin: one uint32 per element.  Returns
        (out limbs, out words (rows, 4 * words_per_row), flag per element)."""
        acc = np.ascontiguousarray(acc, dtype=np.int32)
        sec = None if sec is None else np.ascontiguousarray(sec, dtype=np.int32)
        pt = None if pt is None else np.ascontiguousarray(pt, dtype=np.uint32)
        rows = acc.shape[0]
        n = rows // rows_per_element
        fin = None if fin is None else np.ascontiguousarray(fin, dtype=np.uint32)
        if rows % rows_per_element or (sec is not None and sec.shape != acc.shape) or \
                (pt is not None and pt.shape != (rows, 2 * words_per_row)) or (fin is not None and fin.shape != (n,)):
            raise ValueError("operand arrays of the wrong shape")
        out = np.zeros_like(acc)
        outw = np.zeros((rows, 4 * words_per_row), dtype=np.uint32)
        fout = np.zeros(n, dtype=np.uint32)
        ptrs = self._dev_arrays(acc, sec, pt, fin, out, outw, fout)
        try:
            self._check(self.lib.amdmsm_xyzz_rr_probe_device(self.h, curve, group, int(op), *ptrs, ctypes.c_size_t(n)),
                        "amdmsm_xyzz_rr_probe_device")
            self.d2h(out, ptrs[4])
            self.d2h(outw, ptrs[5])
            self.d2h(fout, ptrs[6])
        finally:
            for p in ptrs:
                if p is not None:
                    self.free(p)
        return out, outw, fout

    def group_op(self, curve, group, op, a, b=None, out_form=OUT_LIBFF):
        """group op over arrays of libff records: 0 add 1 mixed_add 2 dbl"""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
        out = np.zeros_like(a)
        pa, pb, po = self._dev_arrays(a, b, out)
        try:
            self._check(self.lib.amdmsm_group_op_device(self.h, curve, group, op, pa, pb, po,
                                                        ctypes.c_size_t(a.shape[0]), out_form),
                        "amdmsm_group_op_device")
            self.d2h(out, po)
        finally:
            for p in (pa, pb, po):
                if p is not None:
                    self.free(p)
        return out

    def endomorphism_digits(self, curve, group, scalars, c, num_windows, scalars_plain=False):
        """device recoding of both halves of every scalar: int32 (n, 2, num_windows)"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        n = scalars.shape[0]
        out = np.zeros((n, 2, num_windows), dtype=np.int32)
        ps, po = self._dev_arrays(scalars, out)
        try:
            self._check(self.lib.amdmsm_endomorphism_digits_device(self.h, curve, group, ps, ctypes.c_size_t(n),
                                                                   int(scalars_plain), c, num_windows, po),
                        "amdmsm_endomorphism_digits_device")
            self.d2h(out, po)
        finally:
            self.free(ps)
            self.free(po)
        return out

    def signed_digits(self, curve, scalars, c, num_windows, scalars_plain=False):
        """device recoding of every scalar: int32 (n, num_windows), least-significant window first"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        n = scalars.shape[0]
        out = np.zeros((n, num_windows), dtype=np.int32)
        ps, po = self._dev_arrays(scalars, out)
        try:
            self._check(self.lib.amdmsm_digits_device(self.h, curve, G1, ps, ctypes.c_size_t(n), int(scalars_plain),
                                                      c, num_windows, po), "amdmsm_digits_device")
            self.d2h(out, po)
        finally:
            self.free(ps)
            self.free(po)
        return out

    def gen_bases_seq(self, curve, group, n, first=0, as_xyz=True):
        """(first+i+1)*G for i < n, computed on the device; libff special-form records by default"""
        s = sizes(curve, group)
        d_aff = self.malloc(max(16, n * s["affine_bytes"]))
        try:
            self.gen_bases_seq_device(curve, group, first, n, d_aff.value)
            if not as_xyz:
                out = np.zeros((n, s["affine_bytes"] // 8), dtype=np.uint64)
                self.d2h(out, d_aff)
                return out
            d_xyz = self.malloc(max(16, n * s["g_bytes"]))
            try:
                self.export_affine_device(curve, group, d_aff.value, n, d_xyz.value)
                out = np.zeros((n, s["g_bytes"] // 8), dtype=np.uint64)
                self.d2h(out, d_xyz)
                return out
            finally:
                self.free(d_xyz)
        finally:
            self.free(d_aff)
