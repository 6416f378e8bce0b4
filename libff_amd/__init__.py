"""libff_amd -- MI355X-native drop-in for libff's multi_exp (Pippenger/BDLO12) hot path.

Only what the path needs lives here:
  csrc/            hand-written HIP kernels (gfx950) + the C-ABI engine (include/amdmsm.h)
  engine.py        host-side mirror of libff's multi_exp interface over the C ABI (ctypes)
  ffi.py           the FFI-convention entry points (include/libff_amd_ffi.h) over byte buffers
  distributed.py   range-sharded multi-GPU MSM (one process per GPU, RCCL all-gather of partials)
  build.py         hipcc build of libamdmsm.so (in-tree)

There is no CPU implementation in this package: importing is cheap, but every compute
entry raises if libamdmsm.so is missing or no GPU is visible.
"""
from .engine import (  # noqa: F401
    ALT_BN128, BLS12_377, BLS12_381, BW6_761, MNT4, MNT6, G1, G2, OUT_AFFINE, OUT_JACOBIAN, OUT_LIBFF, AmdMsmError, BatchItem, Engine,
    bdlo12_signed_optimal_c, load_library, multi_exp_base_form_normal, multi_exp_base_form_special,
    multi_exp_method_BDLO12, multi_exp_method_BDLO12_signed, multi_exp_method_bos_coster,
    multi_exp_method_naive, multi_exp_method_naive_plain, multi_exp_multi, multi_exp_filter_one_zero_multi, msm_device_multi, pippenger_optimal_c, plan, plan_fold, plan_group_fft, fr_modulus, fft_twiddles, plan_fr_fft, plan_fr_fft_batch, plan_fr_qap_witness_map, fr_root_of_unity, plan_fr_matrix, plan_fr_matrix_transposed, FrMatrix, plan_fr_scan, fr_inverse, fr_domain, fr_domain_element, fr_domain_vanishing, fr_domain_z_terms, fr_multiplicative_generator, plan_sort, plan_sort_digit_grid, plan_write_points, precompute_num_digits, sizes,
    endomorphism_info, plan_short, scalar_desc, ScalarDesc, SCALAR_FR, SCALAR_U8, SCALAR_U16, SCALAR_U32, SCALAR_U64,
    SEG_SHARED_BASES, SEG_LONG_NEVER, SCAN_REVERSE, SCAN_EXCLUSIVE, DOMAIN_BASIC_RADIX2, DOMAIN_STEP_RADIX2)
from . import ffi  # noqa: F401

__all__ = [
    "ALT_BN128", "BLS12_377", "BLS12_381", "BW6_761", "MNT4", "MNT6", "G1", "G2", "OUT_AFFINE", "OUT_JACOBIAN", "OUT_LIBFF",
    "AmdMsmError", "BatchItem", "Engine", "bdlo12_signed_optimal_c", "load_library", "multi_exp_base_form_normal",
    "multi_exp_base_form_special", "multi_exp_method_BDLO12", "multi_exp_method_BDLO12_signed",
    "multi_exp_method_bos_coster", "multi_exp_method_naive", "multi_exp_method_naive_plain", "multi_exp_multi",
    "multi_exp_filter_one_zero_multi", "msm_device_multi",
    "pippenger_optimal_c", "plan", "plan_fold", "plan_group_fft", "fr_modulus", "fft_twiddles", "plan_fr_fft", "plan_fr_fft_batch", "plan_fr_qap_witness_map", "fr_root_of_unity", "plan_fr_matrix", "plan_fr_matrix_transposed", "FrMatrix", "plan_fr_scan", "fr_inverse", "fr_domain", "fr_domain_element", "fr_domain_vanishing", "fr_domain_z_terms", "fr_multiplicative_generator", "plan_sort", "plan_sort_digit_grid", "plan_write_points", "precompute_num_digits", "sizes", "endomorphism_info", "ffi",
    "plan_short", "scalar_desc", "ScalarDesc", "SCALAR_FR", "SCALAR_U8", "SCALAR_U16", "SCALAR_U32", "SCALAR_U64",
    "SEG_SHARED_BASES", "SEG_LONG_NEVER", "SCAN_REVERSE", "SCAN_EXCLUSIVE", "DOMAIN_BASIC_RADIX2", "DOMAIN_STEP_RADIX2",
]
