/* amdmsm -- MI355X (gfx950) multi-scalar-multiplication engine: raw C ABI.
 *
 * This is the drop-in boundary for libff's multi_exp hot path.  Every entry point
 * is `extern "C"` with plain pointers and sizes; no C++ or torch types cross it.
 *
 * What each entry replaces in the reference (clearmatics/libff):
 *   amdmsm_multi_exp          libff::multi_exp<G, Fr, multi_exp_method_BDLO12[_signed], Form>
 *                             multiexp.hpp:63-73, multiexp.tcc:643-688 (and the inner
 *                             Pippenger bodies :284-380, :563-632)
 *   amdmsm_multi_exp_filter_one_zero
 *                             libff::multi_exp_filter_one_zero, multiexp.hpp:78-88,
 *                             multiexp.tcc:690-757
 *   amdmsm_multi_exp_multi    the same multi_exp with libff's chunk split (multiexp.tcc:655-687)
 *                             mapped to the GPUs of one node
 *   amdmsm_register_bases     (extension) keeps a base vector resident in HBM between calls
 *   amdmsm_batch_to_special   libff::batch_to_special<G>, multiexp.hpp:136-141,
 *                             multiexp.tcc:949-974
 *   amdmsm_multi_exp_stream   libff::multi_exp_stream (bases streamed in the on-disk format),
 *                             multiexp_stream.hpp:25-33, multiexp_stream.tcc:164-191
 *   amdmsm_batch_exp          libff::get_window_table + batch_exp / batch_exp_with_coeff,
 *                             multiexp.hpp:99-134, multiexp.tcc:809-947
 *   amdmsm_bdlo12_signed_optimal_c / amdmsm_pippenger_optimal_c
 *                             multiexp.hpp:53-57, multiexp.tcc:35-40, 637-641
 *   amdmsm_*_device           the same path for callers whose vectors already live in
 *                             HBM (proving keys; the benchmark)
 * The FFI-convention wrappers (big-endian plain affine buffers, bool return) that
 * extend ffi/ffi.h:19-95 are declared in include/libff_amd_ffi.h.
 *
 * Data layout at the boundary = libff's in-memory layout, untouched:
 *   scalar   Fp_model<n>: n x uint64 limbs, limb 0 least significant, Montgomery form
 *            (fp.hpp:43).  AMDMSM_SCALARS_PLAIN selects plain bigint<n> instead.
 *   point    G = (X, Y, Z), each coordinate deg*n limbs Montgomery (Fq2: c0 then c1,
 *            fp2.hpp:63); Jacobian for alt_bn128 / bls12_377, homogeneous projective for
 *            bw6_761 -- whatever libff itself uses for the group.
 *   "compact affine" (device-resident bases): (x, y), 2*deg*n limbs, (0,0) = infinity.
 *
 * Errors: every function returns AMDMSM_OK (0) or a negative code; nothing throws and
 * nothing falls back to a CPU path -- without a gfx950 device the calls fail with
 * AMDMSM_ERR_NO_DEVICE.
 */
#ifndef AMDMSM_H
#define AMDMSM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    AMDMSM_CURVE_ALT_BN128 = 0,
    AMDMSM_CURVE_BLS12_377 = 1,
    AMDMSM_CURVE_BW6_761 = 2,
    AMDMSM_CURVE_BLS12_381 = 3,
    /* MNT4-298 / MNT6-298 (libff/algebra/curves/mnt): MNT4 G1 and G2, MNT6 G1.  (MNT6, G2) -- coordinates in
     * Fq3 -- is unsupported everywhere.  No endomorphism: amdmsm_opts.endomorphism is ignored, amdmsm_plan_ex
     * reports endomorphism_used = 0, amdmsm_endomorphism_info and amdmsm_endomorphism_digits_device return
     * AMDMSM_ERR_UNSUPPORTED.  The compressed
     * record paths (amdmsm_multi_exp_stream_compressed[_file], amdmsm_disk_decode_device with compressed = 1)
     * return AMDMSM_ERR_UNSUPPORTED, and the FFI has no MNT names. */
    AMDMSM_CURVE_MNT4 = 4,
    AMDMSM_CURVE_MNT6 = 5
};
enum { AMDMSM_G1 = 1, AMDMSM_G2 = 2 };
/* multi_exp_base_form, multiexp.hpp:45-51 */
enum { AMDMSM_FORM_NORMAL = 0, AMDMSM_FORM_SPECIAL = 1 };
/* result coordinates */
enum {
    AMDMSM_OUT_JACOBIAN = 0, /* engine-internal Jacobian (partial results to be combined) */
    AMDMSM_OUT_LIBFF = 1,    /* libff's coordinate system for the group, not normalised */
    AMDMSM_OUT_AFFINE = 2    /* libff special form: (x, y, 1) or zero = (0, 1, 0) */
};

enum {
    AMDMSM_OK = 0,
    AMDMSM_ERR_NO_DEVICE = -1,
    AMDMSM_ERR_BAD_ARG = -2,
    AMDMSM_ERR_UNSUPPORTED = -3,
    AMDMSM_ERR_HIP = -4,
    AMDMSM_ERR_TOO_LARGE = -5
};

typedef struct amdmsm_ctx amdmsm_ctx;

/* Version of this header's structure layouts and entry points; amdmsm_abi_version() returns the value the
 * loaded library was built with.  3: amdmsm_opts starts with struct_size. */
#define AMDMSM_ABI_VERSION 3

typedef struct amdmsm_opts {
    uint32_t struct_size; /* = sizeof(amdmsm_opts) of the header the caller was compiled against (AMDMSM_OPTS_INIT);
                             a value the library does not know is refused with AMDMSM_ERR_BAD_ARG, so a caller built
                             against another layout fails loudly instead of having its fields misread */
    int window_bits;   /* c; 0 = engine picks (see amdmsm_plan) */
    int segment_len;   /* L for the bucket reduction; 0 = auto */
    int out_form;      /* AMDMSM_OUT_* ; host entry points default to AMDMSM_OUT_LIBFF */
    int scalars_plain; /* nonzero: scalars are plain bigints, not Montgomery residues */
    int endomorphism;  /* k P as k1 P + k2 phi(P), phi(x, y) = (beta x, y), half-length k1, k2: half the windows
                          (bucket reduction and final doublings).  Exact where phi = [lambda], i.e. on the order-r
                          subgroup libff's G1 / G2 are.  0 = permitted only where the whole curve group has order r
                          (alt_bn128 G1), 1 = permitted: the caller guarantees every base lies in that subgroup,
                          2 = same guarantee, used at every size, -1 = never.  Where permitted the engine uses it
                          when it pays (below ~2^22 points; amdmsm_plan_ex tells) */
    void *stream;      /* hipStream_t to launch on (device entry points); NULL = context stream */
} amdmsm_opts;
/* amdmsm_opts o = AMDMSM_OPTS_INIT;  -- every other field zero (= defaults) */
#define AMDMSM_OPTS_INIT { (uint32_t)sizeof(amdmsm_opts) }

#define AMDMSM_MAX_PHASES 8
/* phase indices of amdmsm_get_timings */
enum {
    AMDMSM_PH_COUNT = 0,   /* workspace clears (and the histogram pass of the fallback sort) */
    AMDMSM_PH_SCATTER = 1, /* bucket sort: digits, coarse and fine partition (+ bucket zero-fill) */
    AMDMSM_PH_ACCUM = 2,   /* k_accumulate alone (dominant kernel) */
    AMDMSM_PH_REDUCE = 3,  /* spanning-bucket fix-up + bucket reduction levels */
    AMDMSM_PH_FINAL = 4,   /* Horner over windows */
    AMDMSM_PH_TOTAL = 5
};

int amdmsm_abi_version(void);
int amdmsm_device_count(void);
int amdmsm_ctx_create(int device, amdmsm_ctx **out);
void amdmsm_ctx_destroy(amdmsm_ctx *ctx);
const char *amdmsm_strerror(int code);
/* the message of the context's last refusal; with a NULL context, of the calling thread's last refusal that had none
   (an entry refuses its arguments before it looks at the context) */
const char *amdmsm_last_error(const amdmsm_ctx *ctx);

/* out[0] = sizeof(Fr), out[1] = sizeof(G) (X,Y,Z), out[2] = compact affine bytes, out[3] = Fr bits */
int amdmsm_sizes(int curve, int group, size_t out[4]);

/* window size / round count / bucket count / workspace the engine would use */
int amdmsm_plan(int curve, int group, size_t n, int window_bits, int *c, int *num_windows,
                uint32_t *num_buckets, size_t *workspace_bytes);

/* the same with amdmsm_opts.endomorphism given; *endomorphism_used = 1 when the plan splits the scalars
   (num_windows then covers the half-length scalars and the lists hold 2n columns) */
int amdmsm_plan_ex(int curve, int group, size_t n, int window_bits, int endomorphism, int *c, int *num_windows,
                   uint32_t *num_buckets, size_t *workspace_bytes, int *endomorphism_used);

/* read-only: geometry of the two-level bucket sort the plan above would run (c <= 22).  out[0] = columns per window
   (2n with the split), out[1] = coarse bits, out[2] = fine bits, out[3] = entries of a coarse bin the fine pass sorts in
   one piece (longer bins go chunk by chunk), out[4] = entries above which a coarse bin is spread over the whole grid */
int amdmsm_plan_sort(int curve, int group, size_t n, int window_bits, int endomorphism, size_t out[5]);

/* read-only: the grid of that sort's first pass (the digit pass) over `items` work items -- scalars, or 16-byte vectors
   of packed integers with block_min = 256 -- on a device that holds `workgroups` of its workgroups at once.  Workgroup g
   walks blocks g, g + out[2], ... of out[0] consecutive items: out[0] = items per block, out[1] = blocks, out[2] =
   workgroups launched.  block_min = 0: the workgroup size */
int amdmsm_plan_sort_digit_grid(size_t items, unsigned block_min, unsigned workgroups, size_t out[3]);

/* read-only: the top window of that plan, scalars_plain as in amdmsm_opts.  out[0] = tb, the bits its bucket index
   |digit| - 1 can have -- a bound that holds for every admitted input, never taken from the data: the split's constants,
   or the scalar field's bit length for Montgomery scalars, or the word length for plain ones without the split (k >= r
   is valid input there) -- out[1] = fine bits the sort drops for that window (0 with AMDMSM_SORT_TOPSHIFT=0),
   out[2] = c, out[3] = windows */
int amdmsm_plan_top_window(int curve, int group, size_t n, int window_bits, int endomorphism, int scalars_plain, int out[4]);

/* libff's own window heuristics, kept for API parity (multiexp.hpp:53-57) */
size_t amdmsm_pippenger_optimal_c(size_t num_elements);
size_t amdmsm_bdlo12_signed_optimal_c(size_t num_elements);

/* ---- host-buffer entry points (what the multi_exp<> shim and the FFI call) ---- */
int amdmsm_multi_exp(amdmsm_ctx *ctx, int curve, int group,
                     const void *bases_xyz, size_t base_stride_bytes, int base_form,
                     const void *scalars, size_t n,
                     void *out_xyz, const amdmsm_opts *opts);

int amdmsm_multi_exp_filter_one_zero(amdmsm_ctx *ctx, int curve, int group,
                                     const void *bases_xyz, size_t base_stride_bytes, int base_form,
                                     const void *scalars, size_t n,
                                     void *out_xyz, const amdmsm_opts *opts,
                                     size_t stats[3] /* skipped, ones, other; may be NULL */);

int amdmsm_batch_to_special(amdmsm_ctx *ctx, int curve, int group, void *elems_xyz,
                            size_t stride_bytes, size_t n);

/* Element-wise scalar multiplication of a point vector: out[i] = scalars[i] * points[i], n results -- what a host does
 * with libff's operator* in a loop (an SRS or proving key re-randomised, a powers-of-tau contribution).  One lane per
 * element: a table of the element's multiples 1 P .. 8 P, then a signed 4-bit fixed-window ladder.  points_xyz, stride
 * and base_form as for amdmsm_multi_exp; scalars are Montgomery residues, or with opts->scalars_plain any integers of
 * fr_bytes (values >= r included: the result is the integer multiple); out_xyz receives n packed records in
 * opts->out_form (AMDMSM_OUT_LIBFF by default; AMDMSM_OUT_AFFINE: special form, normalised as amdmsm_batch_to_special
 * does).  The table takes 16 compact affine records of workspace per element, so the vector is worked through
 * chunk_points elements at a time; 0 = as many as fit a workspace of 1 GiB.  n = 0 succeeds and writes nothing.
 * opts->window_bits and opts->endomorphism are accepted and ignored.  With timing enabled, amdmsm_get_timings reports
 * [0] import, [1] table, [2] ladder, [3] normalisation / export -- of the first chunk -- [4] the chunks after it,
 * [AMDMSM_PH_TOTAL] the call. */
int amdmsm_scalar_mul_vec(amdmsm_ctx *ctx, int curve, int group, const void *points_xyz, size_t stride_bytes,
                          int base_form, const void *scalars, size_t n, void *out_xyz,
                          size_t chunk_points, const amdmsm_opts *opts);
/* the same on device-resident inputs: compact affine points (amdmsm_import_bases_device), n records written to
 * d_out_xyz; enqueued on opts->stream (or the context's), not synchronised */
int amdmsm_scalar_mul_vec_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine,
                                 const void *d_scalars, size_t n, void *d_out_xyz,
                                 size_t chunk_points, const amdmsm_opts *opts);

/* Fold of point vectors: k vectors of n points and k scalars give one vector of n points,
 *   out[i] = scalars[0] * P_0[i] + ... + scalars[k-1] * P_(k-1)[i],   i < n,   1 <= k <= 8
 * -- the generator fold of an inner-product round (G'[i] = x^-1 G_lo[i] + x G_hi[i]: k = 2, the halves of one array), a
 * query vector times one scalar (k = 1), a random linear combination of k key or commitment vectors.  The scalars are
 * shared by all elements, so every lane follows the same signed 4-bit digits: one doubling chain serves the k terms, and
 * the windows above the highest nonzero digit of any scalar are skipped (a 128-bit challenge costs half).
 *   points_xyz  k pointers in HOST memory to vectors of libff records; stride_bytes and base_form as for
 *               amdmsm_multi_exp, the same for every vector.  The pointers may alias (one vector twice, the two halves
 *               of one allocation); the output must not overlap an input
 *   scalars     k Fr records in HOST memory (in the device entry too): Montgomery residues, or with opts->scalars_plain
 *               any integers of fr_bytes (a value >= r means the multiple mod r, as in amdmsm_scalar_mul_vec)
 *   out_xyz     n packed records in opts->out_form (AMDMSM_OUT_LIBFF by default; AMDMSM_OUT_AFFINE: special form,
 *               normalised as amdmsm_batch_to_special does)
 * opts->endomorphism follows the permission rule of the MSM (-1 never, 0 only where the whole curve group has order r,
 * 1 / 2 the caller guarantees subgroup points, never for the MNT groups, AMDMSM_GLV=off honoured); where permitted the
 * split is always used, whatever the size: phi(P)'s table is P's with x scaled, so 2k half-length digit rows share half
 * the doublings (amdmsm_plan_fold tells).  opts->window_bits is accepted and ignored.
 * Workspace: the table of amdmsm_scalar_mul_vec for each of the k vectors plus one table's worth of scratch, 8 (k + 1)
 * compact affine records per element, so the vectors are worked through chunk_points elements at a time; 0 = the largest
 * multiple of 256 elements that fits the 1 GiB rule of amdmsm_scalar_mul_vec.
 * AMDMSM_ERR_UNSUPPORTED for (MNT6, G2), before the context is looked at.  AMDMSM_ERR_BAD_ARG, with amdmsm_last_error
 * naming the vector, before anything is launched or written: k outside 1 .. 8, a null pointer array, a null vector,
 * scalar or output pointer with n > 0, a bad stride, a wrong opts->struct_size.  n = 0 succeeds and writes nothing.
 * With timing enabled: [0] import (with the upload), [1] digits and tables, [2] ladder, [3] normalisation / export --
 * of the first chunk -- [4] the chunks after it, [AMDMSM_PH_TOTAL] the call. */
int amdmsm_fold_vec(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *points_xyz, size_t stride_bytes,
                    int base_form, const void *scalars, size_t n, void *out_xyz, size_t chunk_points,
                    const amdmsm_opts *opts);
/* the same on device-resident inputs: k pointers (the array in host memory) to compact affine vectors in device memory
 * (amdmsm_import_bases_device), n records written to d_out_xyz; enqueued on opts->stream (or the context's), not
 * synchronised.  Rounds chain on the device: fold with AMDMSM_OUT_AFFINE, then amdmsm_import_bases_device(d_out_xyz,
 * form special) gives the compact affine vector the next round folds (or its MSM reads). */
int amdmsm_fold_vec_device(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *d_points_affine,
                           const void *scalars, size_t n, void *d_out_xyz, size_t chunk_points,
                           const amdmsm_opts *opts);
/* read-only, no context: out[0] = digit rows (k, or 2k with the split), out[1] = windows per row, out[2] = endomorphism
   used (0/1), out[3] = elements per chunk for (n, chunk_points), out[4] = workspace bytes */
int amdmsm_plan_fold(int curve, int group, int k, size_t n, size_t chunk_points, int endomorphism, size_t out[5]);

/* Radix-2 FFT over a vector of group elements:
 *   out[j] = sum over i < n of w^(i j) * P_i,   j < n,   n a power of two, at most 2^28
 * -- what a host does with libfqfft's radix-2 butterflies on libff group elements: a powers-of-tau SRS brought into
 * Lagrange form (a KZG setup, the phase-2 setup of a Groth16 ceremony).  log2 n autosorting decimation-in-time stages of
 * n / 2 butterflies (A, B, w) -> (A + w B, A - w B), one lane per butterfly: the table of B's multiples 1 B .. 8 B and the
 * signed 4-bit ladder of amdmsm_scalar_mul_vec, then two complete mixed additions.  The first stage, whose twiddles are
 * all 1, has no ladder: n / 2 (log2 n - 1) scalar multiplications in all.  Between stages the n results are normalised
 * as a batch, as amdmsm_batch_to_special does.
 *   points      n records.  Host entry: libff records, stride_bytes and base_form as for amdmsm_multi_exp.  Device entry:
 *               compact affine records in device memory (amdmsm_import_bases_device)
 *   twiddles    n / 2 Fr records w^0 .. w^(n/2 - 1), w a primitive n-th root of unity in Fr (w^(n/2) = -1): Montgomery
 *               residues, or with opts->scalars_plain plain integers of fr_bytes (any integer: a value >= r means itself
 *               mod r).  Host memory for the host entry, device memory for the device entry; may be NULL when n <= 2.
 *               The library has no Fr multiplication and does not check that they are such powers: with other values
 *               the result is unspecified, but the call stays memory-safe and writes only out
 *   out_xyz     n packed records in natural order, in opts->out_form (AMDMSM_OUT_LIBFF by default; AMDMSM_OUT_AFFINE:
 *               special form, normalised as amdmsm_batch_to_special does).  It must not overlap an input
 * n = 0 succeeds and writes nothing, n = 1 copies the point (in special form, whichever form is asked for), n = 2 is one
 * add / sub pair.  There is no inverse flag and no scale argument: the inverse transform is the same call with the
 * powers of w^-1, followed by amdmsm_fold_vec[_device] with k = 1 and the scalar n^-1.  On the device that chain is
 * amdmsm_group_fft_device with AMDMSM_OUT_AFFINE, amdmsm_import_bases_device(d_out_xyz, form special), then the fold --
 * the chain of amdmsm_fold_vec_device's rounds.
 * Workspace: two vectors of n compact affine records and one of n libff records, plus, per butterfly of a chunk, the 16
 * records of amdmsm_scalar_mul_vec's table and scratch and one gathered operand -- so a stage is worked through
 * chunk_points butterflies at a time; 0 = the largest multiple of 256 butterflies whose chunk part fits the 1 GiB rule
 * of amdmsm_scalar_mul_vec, a caller's value is taken as given; never more than n / 2 (amdmsm_plan_group_fft tells).
 * opts->window_bits and opts->endomorphism are accepted and ignored.
 * AMDMSM_ERR_UNSUPPORTED for (MNT6, G2), before the context is looked at.  AMDMSM_ERR_BAD_ARG, with amdmsm_last_error
 * saying which condition, before anything is launched or written: n not a power of two, a null points / out pointer
 * with n > 0, null twiddles with n > 2, a bad stride, a wrong opts->struct_size.  AMDMSM_ERR_TOO_LARGE for n > 2^28.
 * With timing enabled, summed over all stages and chunks of the context's last transform: [0] import (host entry: with
 * the upload), [1] gathers and tables, [2] ladders and butterflies, [3] normalisations and export (host entry: with the
 * download), [AMDMSM_PH_TOTAL] the call. */
int amdmsm_group_fft(amdmsm_ctx *ctx, int curve, int group, const void *points_xyz, size_t stride_bytes, int base_form,
                     size_t n, const void *twiddles, void *out_xyz, size_t chunk_points, const amdmsm_opts *opts);
/* the same on device-resident inputs; enqueued on opts->stream (or the context's), not synchronised */
int amdmsm_group_fft_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n,
                            const void *d_twiddles, void *d_out_xyz, size_t chunk_points, const amdmsm_opts *opts);
/* read-only, no context: out[0] = stages (log2 n), out[1] = stages that run a ladder (max(log2 n - 1, 0)), out[2] =
   scalar multiplications in total (n / 2 * out[1]), out[3] = butterflies per chunk for (n, chunk_points), out[4] =
   workspace bytes, out[5] = the part of out[4] that scales with the chunk.  AMDMSM_ERR_BAD_ARG for n not a power of
   two, AMDMSM_ERR_UNSUPPORTED for (MNT6, G2), AMDMSM_ERR_TOO_LARGE above 2^28 */
int amdmsm_plan_group_fft(int curve, int group, size_t n, size_t chunk_points, size_t out[6]);
/* the scalar-field modulus r of the group: fr_bytes, little-endian words, plain integer; no context */
int amdmsm_fr_modulus(int curve, int group, void *r_plain);

/* Radix-2 FFT over a vector of Fr scalars -- the transforms in front of a prover's large MSMs, so that the scalars stay
 * in device memory from the witness evaluations to the MSM result:
 *   out[j] = post^j * scale * sum over i < n of pre^i * a_i * w^(i j),   j < n,   n a power of two, at most 2^28
 * Fr belongs to the curve, so these entries take no group; all six curve ids are served, AMDMSM_CURVE_MNT6 included.
 *   values, out  n Fr records of fr_bytes (amdmsm_sizes of the curve's G1), natural order in and out: libff's in-memory
 *                Fr, canonical Montgomery residues below r, or with opts->scalars_plain plain integers below r -- the
 *                data, the output and the four parameters alike; the conversion happens at the first load and the last
 *                store.  A record >= r gives an unspecified value; it never causes an access outside out.
 *                Device entry: d_out == d_values is allowed (the transform then runs in place); any other overlap of
 *                the two ranges is AMDMSM_ERR_BAD_ARG.  The kernels move the 32- and 48-byte records 16 bytes at a
 *                time and the 40-byte records of MNT4 / MNT6 8 bytes at a time: d_values and d_out must be aligned to
 *                16 and 8 bytes respectively (what amdmsm_malloc and hipMalloc return is), or the call is
 *                AMDMSM_ERR_BAD_ARG; the same holds for the device vectors of amdmsm_fr_powers_device and
 *                amdmsm_fr_muladd_device.  The host entry's arrays need no alignment
 *   omega        a primitive n-th root of unity, one record in host memory (amdmsm_fr_root_of_unity gives libff's); may
 *                be NULL when n <= 1.  Checked on the host: omega^(n/2) must be r - 1
 *   pre, post, scale   one record each in host memory, NULL = 1.  All NULL: libfqfft's FFT.  pre = g: the coset FFT by
 *                g.  omega^-1 and scale = n^-1: the inverse FFT; with post = g^-1 as well: the inverse coset FFT.
 *                amdmsm_fr_inverse gives the inverses
 *   tile_log2    butterfly stages of one global pass, 0 = the default; amdmsm_plan_fr_fft reports the range
 * A transform is ceil(log2 n / tile) passes; a pass reads every record once and writes it once, pre^i is applied as the
 * first pass loads and post^j * scale as the last pass stores.  Workspace, from the context's slots: one vector of n
 * records (two for an in-place call of an odd number of passes above one; the host entry adds the uploaded vector),
 * and the powers of pre and post a pass needs: (n >> stages) + 2^stages records of its first / last pass.  The n / 2
 * powers of omega are kept with the context for the last four (curve, n, omega) it served and freed with it.
 * n = 0 succeeds and writes nothing; n = 1 writes scale * a_0.
 * AMDMSM_ERR_UNSUPPORTED for an unknown curve.  AMDMSM_ERR_BAD_ARG, with amdmsm_last_error naming the condition, before
 * anything is launched or written: n not a power of two, a null vector pointer with n > 0, null omega with n > 1, an
 * omega with omega^(n/2) != r - 1 (which every n above the field's 2-adicity fails), a nonzero tile_log2 outside the
 * plan's range, a wrong opts->struct_size, ranges that overlap without being equal, a misaligned device vector.  AMDMSM_ERR_TOO_LARGE for
 * n > 2^28.  These are looked at before the context is.
 * With timing enabled (amdmsm_get_timings): [0] the powers of omega, pre and post (host entry: with the upload), [1] the
 * passes, [2] the download (host entry), [AMDMSM_PH_TOTAL] the call. */
int amdmsm_fr_fft(amdmsm_ctx *ctx, int curve, const void *values, size_t n, const void *omega, const void *pre,
                  const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, void *out);
/* the same on device-resident vectors (omega, pre, post, scale stay in host memory); enqueued on opts->stream (or the
   context's), not synchronised */
int amdmsm_fr_fft_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t n, const void *omega, const void *pre,
                         const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, void *d_out);
/* read-only, no context: out[0] = tile (log2) in use, out[1] / out[2] = smallest / largest tile the unit supports,
   out[3] = global passes, out[4] = butterflies (n / 2 * log2 n), out[5] = workspace bytes of an out-of-place device
   call with pre and post given.  AMDMSM_ERR_BAD_ARG for n not a power of two or a tile out of range,
   AMDMSM_ERR_TOO_LARGE above 2^28 */
int amdmsm_plan_fr_fft(int curve, size_t n, int tile_log2, size_t out[6]);
/* The same transform over `batch` vectors of n records with one set of parameters: the A, B and C of a witness map, the
 * columns of a trace, the rows of a two-dimensional transform.  Every vector gets exactly the records amdmsm_fr_fft_device
 * gives it alone, bit for bit, in both record forms and with pre / post / scale; the batch goes through one chain of
 * passes (k_fr_fft_pass_batch) whose grid covers all vectors: batch * n / 2^10 workgroups from
 * n = 2^10 on, and below that ceil(batch / V) workgroups that hold V = 2^10 / n whole vectors each.
 *   d_values, d_out   vector v starts in_stride * v records into d_values and out_stride * v records into d_out; the
 *                     records between the vectors are neither read nor written.  d_out == d_values with equal strides
 *                     runs in place; any other overlap of the ranges [d, d + ((batch - 1) * stride + n) records) is
 *                     AMDMSM_ERR_BAD_ARG.  Alignment as for amdmsm_fr_fft_device (a stride in records keeps it).  The
 *                     host entry takes and gives packed vectors (stride n)
 *   batch * n         at most 2^28; batch = 0 and n = 0 succeed and write nothing
 * Workspace, from the context's slots: batch vectors of n records (two such sets for an in-place call of an odd number
 * of passes above one; the host entry adds the uploaded set), one copy of the powers of pre and post, and the n / 2
 * powers of omega from the context's cache.
 * Refused before anything is launched or written and before the context is looked at, amdmsm_last_error naming the
 * argument: everything amdmsm_fr_fft_device refuses, with its code and message; AMDMSM_ERR_TOO_LARGE for batch * n > 2^28
 * and for a stride with which the batch does not fit size_t; AMDMSM_ERR_BAD_ARG for a stride below n with batch > 1,
 * overlapping ranges and misaligned vectors.  Timing phases as for amdmsm_fr_fft_device. */
int amdmsm_fr_fft_batch_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t n, size_t batch, size_t in_stride,
                               size_t out_stride, const void *omega, const void *pre, const void *post, const void *scale,
                               int tile_log2, const amdmsm_opts *opts, void *d_out);
int amdmsm_fr_fft_batch(amdmsm_ctx *ctx, int curve, const void *values, size_t n, size_t batch, const void *omega, const void *pre,
                        const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, void *out);
/* read-only, no context: out[0] = tile (log2) in use, out[1] = global passes, out[2] = vectors of one workgroup (2^10 / n
   below 2^10 records, else 1), out[3] = workgroups of a pass, out[4] = launches of the pass kernel, out[5] = butterflies,
   out[6] / out[7] = workspace bytes of an out-of-place / in-place device call with pre and post given.  Codes as
   amdmsm_plan_fr_fft, AMDMSM_ERR_TOO_LARGE also for batch * n > 2^28 */
int amdmsm_plan_fr_fft_batch(int curve, size_t n, size_t batch, int tile_log2, size_t out[8]);
/* libff's get_root_of_unity<Fr>(2^log2_n) -- Fr::root_of_unity squared s - log2_n times, s the 2-adicity of r - 1 -- as
   a plain integer of fr_bytes; no context.  AMDMSM_ERR_BAD_ARG beyond s */
int amdmsm_fr_root_of_unity(int curve, int log2_n, void *r_plain_out);
/* d_out[i] = base^i, i < n (any n): the builder of the transform's twiddles, which also gives amdmsm_group_fft_device
   its twiddles and amdmsm_scalar_mul_vec_device the powers of a coset generator.  base: one record in host memory;
   records in the form opts->scalars_plain says.  Enqueued, not synchronised */
int amdmsm_fr_powers_device(amdmsm_ctx *ctx, int curve, const void *base, size_t n, const amdmsm_opts *opts, void *d_out);
/* d_out[i] = (a_i * b_i - c_i) * k, i < n: the element-wise step between the coset transforms of a quotient.  d_c and k
   (one record in host memory) may be NULL: 0 and 1.  d_out may be any of the inputs.  Enqueued, not synchronised */
int amdmsm_fr_muladd_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_a, const void *d_b, const void *d_c,
                            const void *k, const amdmsm_opts *opts, void *d_out);
/* d_out[i] = sum over j < k of s_j * v_j[i], i < n: a linear combination of 1 <= k <= 4 resident vectors with scalars
   from the host -- the key vectors (beta At + alpha Bt + Ct) / delta of a generator, the blinding terms of a witness
   map.  d_v: k device vectors, listed in host memory; scalars: k packed records in host memory; vectors and scalars in
   the form opts->scalars_plain says, n <= 2^28.  d_out may be any one of the v_j as a whole (a vector may also be listed
   twice); any other overlap with d_out is refused.  One lane per record, one launch; enqueued, not synchronised.
   AMDMSM_ERR_BAD_ARG, before anything is launched and before the context is looked at, for k out of range, a scalar not
   below r, a null scalars or d_v, and with n > 0 a null or misaligned vector; n = 0 succeeds and writes nothing.  With
   timing enabled: [1] the kernel */
int amdmsm_fr_lincomb_device(amdmsm_ctx *ctx, int curve, size_t n, int k, const void *const *d_v, const void *scalars,
                             const amdmsm_opts *opts, void *d_out);

/* Scans and batch inversion over a vector of Fr records -- the operations that carry a value from one record to the
 * next: prefix products (the z vector of a grand product), prefix sums, Horner evaluation and synthetic division by
 * X - z in front of an opening, Lagrange coefficients.  Records as for amdmsm_fr_fft: Montgomery residues below r, or
 * with opts->scalars_plain plain integers below r, the vectors, a_const, init and the total alike; a record >= r gives
 * unspecified values in the outputs that depend on it and never an access outside the outputs.
 * Scan: the first-order recurrence over n <= 2^28 records
 *     y_(-1) = init,  y_i = a_i * y_(i-1) + b_i,  i = 0 .. n - 1;        total = y_(n-1)
 *     out[i] = y_i, or with AMDMSM_SCAN_EXCLUSIVE y_(i-1) (out[0] = init)
 * and with AMDMSM_SCAN_REVERSE from the other end: y_n = init, y_i = a_i * y_(i+1) + b_i, i = n - 1 .. 0, total = y_0,
 * out[i] = y_i or, exclusive, y_(i+1).
 *   a        a vector (d_a / a), or one record in host memory for every i (a_const), or neither: every a_i is 1
 *   b        a vector (d_b / b) or NULL: every b_i is 0
 *   init     one record in host memory; NULL means 1 without b and 0 with it
 *   total    one record (d_total in HBM / total in host memory), may be NULL.  n = 0 writes nothing but total = init
 * d_a alone: prefix products.  d_b alone: prefix sums.  a_const = z, d_b = p, reverse, exclusive, init = 0: out[i] is
 * coefficient i of (p(X) - p(z)) / (X - z), out[n - 1] = 0 and total = p(z).
 * Batch inversion: out[i] = 1 / values[i], and 0 where values[i] is 0; the number of zero records goes to
 * d_zero_count (a uint64 in HBM, aligned to 8 bytes) / zero_count (host memory), which may be NULL and need not be
 * cleared.  One field inversion per call, whatever n.
 *   tile_log2   records of one workgroup's tile (log2), 0 = the default; amdmsm_plan_fr_scan reports the range
 * Device entries: enqueued on opts->stream (or the context's), not synchronised.  d_out may be exactly d_a, d_b or
 * d_values (a tile loads all it needs before it stores); any other overlap is refused, as is a d_total or d_zero_count
 * inside a vector.  Vectors and d_total aligned as the vectors of amdmsm_fr_fft_device.  The host entries (no alignment
 * rule) upload, run, download and synchronise.
 * Three launches in stream order and no kernel that waits for another workgroup: every tile's aggregate, one workgroup
 * over the aggregates, every tile again.  AMDMSM_FR_SCAN_NAIVE=1 in the environment of a call has
 * one lane walk the vector instead: the second implementation the tests compare with and the baseline of
 * profiles/fr_scan.txt.
 * Refused before anything is launched or written and before the context is looked at, amdmsm_last_error naming the
 * argument: AMDMSM_ERR_UNSUPPORTED for an unknown curve; AMDMSM_ERR_TOO_LARGE for n > 2^28; AMDMSM_ERR_BAD_ARG for a
 * wrong opts->struct_size, unknown flag bits, d_a and a_const both given, a and b both absent, a null or misaligned
 * vector with n > 0, a partial overlap, a nonzero tile_log2 outside the plan's range, a_const or init not below r.
 * With timing enabled (amdmsm_get_timings): [0] the upload (host entries), [1] the kernels, [2] the download (host
 * entries), [AMDMSM_PH_TOTAL] the call. */
#define AMDMSM_SCAN_REVERSE 1
#define AMDMSM_SCAN_EXCLUSIVE 2
int amdmsm_fr_scan_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_a, const void *a_const, const void *d_b,
                          const void *init, int flags, int tile_log2, const amdmsm_opts *opts, void *d_out, void *d_total);
int amdmsm_fr_scan(amdmsm_ctx *ctx, int curve, size_t n, const void *a, const void *a_const, const void *b, const void *init,
                   int flags, int tile_log2, const amdmsm_opts *opts, void *out, void *total);
int amdmsm_fr_batch_invert_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_values, int tile_log2,
                                  const amdmsm_opts *opts, void *d_out, uint64_t *d_zero_count);
int amdmsm_fr_batch_invert(amdmsm_ctx *ctx, int curve, size_t n, const void *values, const amdmsm_opts *opts, void *out,
                           uint64_t *zero_count);
/* What a scan or an inversion of n records runs, read-only and without a context.  kind_and_flags: what is given --
 * AMDMSM_SCAN_KIND_A (a vector or a_const) and / or AMDMSM_SCAN_KIND_B, with the scan's flags, or AMDMSM_SCAN_KIND_INVERT
 * alone.
 *   out[0]  records of a tile      out[1]  records of a lane      out[2]  tiles the spine takes per step
 *   out[3] / out[4]  smallest / largest tile_log2                 out[5]  launches
 *   out[6]  workspace bytes        out[7]  field products per record, the block scans' share left out
 * (AMDMSM_FR_SCAN_NAIVE=1: one launch; an inversion keeps n records of workspace).  AMDMSM_ERR_BAD_ARG for a kind that
 * names nothing, unknown bits or a tile out of range, AMDMSM_ERR_TOO_LARGE above 2^28 */
#define AMDMSM_SCAN_KIND_A 0x100
#define AMDMSM_SCAN_KIND_B 0x200
#define AMDMSM_SCAN_KIND_INVERT 0x400
int amdmsm_plan_fr_scan(int curve, size_t n, int kind_and_flags, int tile_log2, size_t out[8]);
/* out = 1 / x in Fr, one record in host memory each, Montgomery residues or with plain != 0 plain integers; one Fermat
   power on the host, no context: n^-1, g^-1 and omega^-1 of an inverse transform.  AMDMSM_ERR_BAD_ARG for 0 and for a
   value not below r */
int amdmsm_fr_inverse(int curve, const void *x, int plain, void *out);

/* Evaluation domains over Fr as libfqfft chooses them -- what libsnark's r1cs_to_qap_witness_map gets from
 * get_evaluation_domain(num_constraints + num_inputs + 1), a size that is hardly ever a power of two -- and on them the
 * transforms, the vanishing polynomial and the division by it on a coset: a quotient whose H-query belongs to a step
 * radix-2 domain stays on the device.  Restated from libfqfft's step_radix2_domain and get_evaluation_domain, not checked
 * against its code: the point sets and their order below are the contract.  root(n) is amdmsm_fr_root_of_unity, log2 the
 * ceiling log, s the 2-adicity of r - 1.
 * Choice, min_size >= 2: big = 2^(log2(min_size) - 1), small = min_size - big, rounded = 2^log2(small).  min_size a
 * power of two: the basic radix-2 domain of min_size.  Else small a power of two: the step domain of min_size.  Else
 * big + rounded a power of two: the basic domain of it.  Else the step domain of big + rounded.
 *   basic, m points:      x_j = root(m)^j;                                   Z = X^m - 1;      needs log2 m <= s
 *   step, m = B + S, B and S powers of two, S < B, w = root(2 B), sigma = root(S):
 *                         x_j = w^(2 j), j < B;  x_j = w sigma^(j - B), B <= j < m;
 *                         Z = (X^B - 1) (X^S - w^S);                                           needs log2(2 B) <= s
 * Where libfqfft would go on to its extended radix-2 domain (m = 2^(s + 1): MNT6 at 2^18) or to a geometric sequence
 * (everything else above 2^s on MNT6) the answer is AMDMSM_ERR_UNSUPPORTED, the message of an entry with a context naming
 * that domain; min_size < 2 is AMDMSM_ERR_BAD_ARG, m > 2^28 AMDMSM_ERR_TOO_LARGE.
 *
 * amdmsm_fr_domain: out[0] = the kind, out[1] = m, out[2] = B (m for a basic domain), out[3] = S (0 for a basic domain),
 * out[4] = log2 of the order of w, out[5] = workspace bytes of an out-of-place device transform with a coset.
 * amdmsm_fr_domain_element: x_idx.  amdmsm_fr_domain_vanishing: Z(t).  amdmsm_fr_domain_z_terms: Z as *count <= 4 pairs
 * (idx[k], coefficient k), the highest index first -- what libfqfft's add_poly_Z adds, times a constant, to a
 * coefficient vector.  amdmsm_fr_multiplicative_generator: libff's Fr::multiplicative_generator, the coset shift of a
 * quotient.  One record in host memory each, Montgomery residues or with plain != 0 plain integers; no context; the
 * four entries that take m answer AMDMSM_ERR_BAD_ARG for an m that amdmsm_fr_domain would not answer with. */
#define AMDMSM_DOMAIN_BASIC_RADIX2 0
#define AMDMSM_DOMAIN_STEP_RADIX2 1
int amdmsm_fr_domain(int curve, size_t min_size, size_t out[6]);
int amdmsm_fr_domain_element(int curve, size_t m, size_t idx, int plain, void *out);
int amdmsm_fr_domain_vanishing(int curve, size_t m, const void *t, int plain, void *out);
int amdmsm_fr_domain_z_terms(int curve, size_t m, int plain, size_t idx[4], void *coeffs, int *count);
int amdmsm_fr_multiplicative_generator(int curve, int plain, void *out);
/* The transform over the domain of m points, records and device vectors as for amdmsm_fr_fft:
 *   forward   out[j] = A(g x_j), A(X) = sum over i < m of values[i] X^i
 *   inverse   (AMDMSM_DOMAIN_INVERSE) out = the m coefficients of the A of degree < m with A(g x_j) = values[j]
 *   coset     g, one record in host memory, NULL = 1; tile_log2 as for amdmsm_fr_fft, for the passes
 * A basic domain is amdmsm_fr_fft with libff's root.  A step domain is one sweep in front of (the fold) or behind (the
 * merge) radix-2 transforms of B and of S records, which are amdmsm_fr_fft's passes: the sweep reads the m records once,
 * applies g^i and w^i, converts plain records, and sums the K = B / S rows of a K x S matrix column by column -- over
 * lanes and workgroups, the partial sums by further launches in stream order; no kernel waits for another workgroup
 * (DESIGN section 22).  Workspace from the context's slots (amdmsm_fr_domain reports it); the B powers of w and the powers
 * of the two transforms stay in the context's cache of four.
 * amdmsm_fr_domain_divide_by_z: out[j] = values[j] / Z(g x_j), the step between the coset transform and the inverse
 * coset transform of a quotient; coset is required.  Below B the denominator takes K values, built on the device and
 * inverted by the batch inversion above; from B on, and for a basic domain, it is one value, inverted on the host.
 * Device entries: enqueued on opts->stream (or the context's), not synchronised; d_out may be d_values, any other overlap
 * is refused.  The host entries upload, run, download and synchronise.
 * Refused before anything is launched or written and before the context is looked at, amdmsm_last_error naming the
 * argument: AMDMSM_ERR_UNSUPPORTED for an unknown curve and the domains left out; AMDMSM_ERR_TOO_LARGE for m > 2^28;
 * AMDMSM_ERR_BAD_ARG for an m that is no domain size (the message names the size amdmsm_fr_domain chooses), m < 2, a
 * null or misaligned vector, a partial overlap, unknown flags, a tile_log2 out of range, a wrong opts->struct_size, a
 * coset not below r or zero, and for the division a missing coset or one with g^(2 B) = 1 (step) or g^m = 1 (basic),
 * where Z has a zero.
 * With timing enabled (amdmsm_get_timings): [0] the powers (host entries: with the upload), [1] the kernels, [2] the
 * download (host entries), [AMDMSM_PH_TOTAL] the call. */
#define AMDMSM_DOMAIN_INVERSE 1
int amdmsm_fr_domain_fft(amdmsm_ctx *ctx, int curve, const void *values, size_t m, int flags, const void *coset, int tile_log2,
                         const amdmsm_opts *opts, void *out);
int amdmsm_fr_domain_fft_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t m, int flags, const void *coset,
                                int tile_log2, const amdmsm_opts *opts, void *d_out);
int amdmsm_fr_domain_divide_by_z(amdmsm_ctx *ctx, int curve, size_t m, const void *values, const void *coset,
                                 const amdmsm_opts *opts, void *out);
int amdmsm_fr_domain_divide_by_z_device(amdmsm_ctx *ctx, int curve, size_t m, const void *d_values, const void *coset,
                                        const amdmsm_opts *opts, void *d_out);
/* The Lagrange vector of the domain of m points at a point t -- what libfqfft's evaluate_all_lagrange_polynomials(t)
 * answers, the u of libsnark's r1cs_to_qap_instance_map_with_evaluation, and the weights that evaluate a polynomial held
 * in evaluation form, A(t) = sum over j of L_j(t) A(x_j):
 *     out[j] = L_j(t) = product over k != j of (t - x_k) / (x_j - x_k),   j < m,
 * on the points x_j above, in their order; for t = x_k the unit vector e_k.  Restated from that property, not checked
 * against libfqfft's code: the point order is the contract.
 *   t   one record in host memory in the form opts->scalars_plain says, as the coset of amdmsm_fr_domain_fft; any
 *       value below r, 0 and the points of the domain included.  The results are in the same form
 * With Z(t) != 0 one sweep writes the m denominators 1 / L_j(t) -- (t / x_j - 1) times m / Z(t) on a basic domain; on a
 * step domain times B (rho^(j mod K) - w^S) / Z(t) below B, rho = w^(2 S), K = B / S, and times -2 S w^S / Z(t) from B
 * on -- from the cached powers of w and K factors built as those of the division by Z, and the batch inversion above
 * inverts them in place: one field inversion on the device and one, of Z(t), on the host, whatever m (DESIGN section
 * 24).  With Z(t) = 0 the same sweep compares x_j with t and writes the unit vector; nothing is inverted.
 * The device entry is enqueued on opts->stream (or the context's) and not synchronised, d_out aligned as the vectors of
 * amdmsm_fr_fft_device; the host entry runs, downloads and synchronises.  Workspace from the context's slots.
 * Refused before anything is launched or written and before the context is looked at, amdmsm_last_error naming the
 * argument: AMDMSM_ERR_UNSUPPORTED for an unknown curve and the domains left out; AMDMSM_ERR_TOO_LARGE for m > 2^28;
 * AMDMSM_ERR_BAD_ARG for an m that is no domain size (the message names the size amdmsm_fr_domain chooses), m < 2, a
 * null t or output, a t not below r, a misaligned d_out, a wrong opts->struct_size.
 * With timing enabled (amdmsm_get_timings): [0] the tables, [1] the kernels, [2] the download (host entry),
 * [AMDMSM_PH_TOTAL] the call. */
int amdmsm_fr_domain_lagrange_device(amdmsm_ctx *ctx, int curve, size_t m, const void *t, const amdmsm_opts *opts, void *d_out);
int amdmsm_fr_domain_lagrange(amdmsm_ctx *ctx, int curve, size_t m, const void *t, const amdmsm_opts *opts, void *out);
/* amdmsm_fr_domain_fft_device over `batch` vectors of m records, laid out and refused as the vectors of
 * amdmsm_fr_fft_batch_device (a stride below m is refused); every vector gets what the single entry gives it, bit for
 * bit.  On a step domain the radix-2 transforms of B and of S records go through the batched passes; the fold, merge and
 * combine sweeps are enqueued vector by vector.  batch = 0 succeeds and writes nothing. */
int amdmsm_fr_domain_fft_batch_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t m, size_t batch, size_t in_stride,
                                      size_t out_stride, int flags, const void *coset, int tile_log2, const amdmsm_opts *opts,
                                      void *d_out);

/* libsnark's r1cs_to_qap_witness_map as one call: from the full assignment z and the three constraint matrices, kept on
 * the device by amdmsm_fr_matrix_load (below; the input-consistency rows are rows of A that the caller adds), the
 * m + 1 coefficients of H.  With aA, aB, aC the applies of the three handles on z, zero-filled to m records, A, B, C
 * the polynomials of degree < m with those values on the domain of m points, Z its vanishing polynomial:
 *     (A + d1 Z) (B + d2 Z) - (C + d3 Z) = H Z,    H = (A B - C) / Z + d2 A + d1 B + d1 d2 Z - d3
 *   m       a size amdmsm_fr_domain answers with, at most 2^28; every handle has at most m rows
 *   d_z     n_z records, n_z at least the columns of every handle;  d_h  m + 1 records, not overlapping d_z
 *   blind   d1, d2, d3: three packed records in host memory, or NULL for none (libsnark's Groth16 prover); then
 *           h[m - 1] = h[m] = 0
 * Records -- z, h and the blinding -- in the form opts->scalars_plain says.  One slot of workspace (three vectors of m
 * records, the batched transform's and the division's workspace; amdmsm_plan_fr_qap_witness_map reports it without the
 * applies' partial sums) and this chain on one stream: three applies, one batch of three inverse transforms, with
 * blinding d2 A + d1 B, one batch of three coset transforms by amdmsm_fr_multiplicative_generator, a b - c, the division
 * by Z, one inverse coset transform, and the few terms of d1 d2 Z - d3.  The records are those of the twelve single calls.
 * The device entry is enqueued on opts->stream (or the context's) and not synchronised; the host entry uploads z, runs,
 * downloads h and synchronises.
 * Refused before anything is launched or written: AMDMSM_ERR_UNSUPPORTED for an unknown curve and the domains left out;
 * AMDMSM_ERR_TOO_LARGE for m or n_z above 2^28; AMDMSM_ERR_BAD_ARG, amdmsm_last_error naming the argument, for an m that
 * is no domain size, a null or misaligned vector, d_h overlapping d_z, a blinding record not below r, a wrong
 * opts->struct_size -- these before the context is looked at -- and for a handle that is not a live handle of this
 * context or belongs to another curve, a handle with more than m rows, n_z below a handle's columns.
 * With timing enabled: [0] the tables of powers (host entry: with the upload), [1] the kernels, [2] the download (host
 * entry), [AMDMSM_PH_TOTAL] the call.
 * amdmsm_plan_fr_qap_witness_map, read-only and without a context: out[0] = the domain's kind, out[1] = m, out[2] = B,
 * out[3] = S, out[4] = workspace bytes, out[5] = launches of the batched pass kernel. */
int amdmsm_fr_qap_witness_map_device(amdmsm_ctx *ctx, int curve, uint64_t mat_a, uint64_t mat_b, uint64_t mat_c, const void *d_z,
                                     size_t n_z, size_t m, const void *blind, const amdmsm_opts *opts, void *d_h);
int amdmsm_fr_qap_witness_map(amdmsm_ctx *ctx, int curve, uint64_t mat_a, uint64_t mat_b, uint64_t mat_c, const void *z, size_t n_z,
                              size_t m, const void *blind, const amdmsm_opts *opts, void *h);
int amdmsm_plan_fr_qap_witness_map(int curve, size_t m, size_t out[6]);

/* Sparse matrix times Fr vector -- the rows <A_i, z>, <B_i, z>, <C_i, z> of a constraint system on a resident
 * assignment, the vectors the transforms above start from -- and any other sparse linear map over Fr:
 *     out[i] = sum over offsets[i] <= k < offsets[i + 1] of coeffs[k] * x[cols[k]]  (mod r),   i < n_rows
 *     out[i] = 0,                                                                              n_rows <= i < n_out
 * The matrix is given once, in CSR form, and kept in HBM in a form of the library's own; an apply
 * reads the vector and writes canonical records, bit for bit the sum taken with integers.
 *   offsets   n_rows + 1 values, offsets[0] = 0, not decreasing; offsets[n_rows] = nnz <= 2^31
 *   cols      nnz columns below n_cols, in any order within a row; a column may repeat, its terms add
 *   coeffs    nnz Fr records below r: Montgomery residues, or with coeffs_plain != 0 plain integers.  A zero
 *             coefficient contributes nothing (it is dropped at the load)
 *   n_rows, n_cols  at most 2^28 each; 0 rows and 0 entries are valid
 * amdmsm_fr_matrix_load validates the arrays, rearranges them on the host, uploads the result and returns a handle that
 * belongs to the context; it synchronises.  AMDMSM_ERR_UNSUPPORTED for an unknown curve (looked at before the context);
 * AMDMSM_ERR_BAD_ARG, with amdmsm_last_error naming the row or entry, before anything is allocated or uploaded, for
 * offsets[0] != 0, a decreasing offset, a column >= n_cols, a coefficient >= r, a null array with work to do;
 * AMDMSM_ERR_TOO_LARGE above the limits.  AMDMSM_FR_MATRIX_NAIVE=1 in the environment of the load keeps the CSR arrays
 * as they are and has the applies of that handle run one lane per row, a product and an addition per entry: the
 * second implementation the tests compare with, and the baseline of profiles/fr_matrix.txt.
 * amdmsm_fr_matrix_apply_device: d_x (n_x >= n_cols records) and d_out (n_out >= n_rows records) in HBM, both in the
 * form opts->scalars_plain says, aligned as the vectors of amdmsm_fr_fft_device and not overlapping.  Records n_rows ..
 * n_out - 1 are written as zero -- the output is the input of a transform of size n_out as it stands -- and nothing at
 * or beyond n_out is touched.  Enqueued on opts->stream (or the context's), not synchronised; one handle may be applied
 * on several streams.  AMDMSM_ERR_BAD_ARG, with a message, before anything is launched or written: a handle of another
 * context or a freed one, n_x < n_cols, n_out < n_rows, a null vector with work to do, a misaligned or overlapping
 * vector, a wrong opts->struct_size; AMDMSM_ERR_TOO_LARGE for n_x or n_out above 2^28.  A record of x that is not below
 * r gives an unspecified value in the rows that read it and nothing else: every address comes from the validated
 * handle, none from the vector.
 * amdmsm_fr_matrix_apply: the same with x and out in host memory (no alignment rule); uploads, applies, downloads and
 * synchronises.
 * amdmsm_fr_matrix_free waits for the applies that still use the handle and releases it; handles still alive are
 * released with the context.
 * With timing enabled (amdmsm_get_timings): [0] the upload (host entry), [1] the kernels, [2] the download (host
 * entry), [AMDMSM_PH_TOTAL] the call. */
int amdmsm_fr_matrix_load(amdmsm_ctx *ctx, int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets,
                          const uint32_t *cols, const void *coeffs, int coeffs_plain, uint64_t *mat);
int amdmsm_fr_matrix_apply_device(amdmsm_ctx *ctx, uint64_t mat, const void *d_x, size_t n_x, void *d_out, size_t n_out,
                                  const amdmsm_opts *opts);
int amdmsm_fr_matrix_apply(amdmsm_ctx *ctx, uint64_t mat, const void *x, size_t n_x, void *out, size_t n_out,
                           const amdmsm_opts *opts);
int amdmsm_fr_matrix_free(amdmsm_ctx *ctx, uint64_t mat);
/* What amdmsm_fr_matrix_load would build, read-only and without a context; it validates exactly what the load does,
 * with the same codes (the message is not kept).  Rows are classed by the number of their non-zero entries:
 *   out[0]  nnz as given            out[1 .. 4]  entries with a general coefficient / 1 / r - 1 / 0 (dropped)
 *   out[5 .. 7]  rows served one to a lane (shorter than out[8]) / by one wave / by several waves (longer than out[9])
 *   out[8]  the shortest row that takes a wave    out[9]  the longest row one wave takes
 *   out[10] the longest row         out[11] device bytes of the resident form
 *   out[12] launches of one apply   out[13] general products per Montgomery reduction, the field's chain length
 *   out[14] wave jobs of one apply  out[15] partial sums an apply keeps in its workspace
 * AMDMSM_FR_MATRIX_WAVE_ROW / AMDMSM_FR_MATRIX_SPLIT_ROW in the environment replace out[8] / out[9] (experiments). */
#define AMDMSM_FR_MATRIX_PLAN_WORDS 16
int amdmsm_plan_fr_matrix(int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
                          const void *coeffs, int coeffs_plain, size_t out[AMDMSM_FR_MATRIX_PLAN_WORDS]);
/* The transposed map: the arguments are the CSR arrays of a matrix M exactly as amdmsm_fr_matrix_load takes them, the
 * handle is that of its transpose -- n_cols rows and n_rows columns, so that
 *     amdmsm_fr_matrix_apply*(mat, u, n_x >= n_rows, out, n_out >= n_cols):  out[c] = sum over the entries (i, c) of M of coeff * u[i]
 * which with u the Lagrange vector of a domain at t gives At, Bt, Ct of r1cs_to_qap_instance_map_with_evaluation (the
 * input-consistency terms At[i] = u[num_constraints + i] are rows of M the caller adds).  Validation, codes and messages
 * are those of the plain load and name rows and entries of M as given.  A stable counting sort on the host then gives
 * the CSR of the transpose -- within a row the entries in ascending row of M -- through an index per entry, the
 * coefficients are read where the caller has them; zero coefficients are dropped, and from there the handle is an
 * ordinary one in every respect, AMDMSM_FR_MATRIX_NAIVE=1 included.  The plan twin reports what amdmsm_plan_fr_matrix
 * reports for the transpose. */
int amdmsm_fr_matrix_load_transposed(amdmsm_ctx *ctx, int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets,
                                     const uint32_t *cols, const void *coeffs, int coeffs_plain, uint64_t *mat);
int amdmsm_plan_fr_matrix_transposed(int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
                                     const void *coeffs, int coeffs_plain, size_t out[AMDMSM_FR_MATRIX_PLAN_WORDS]);

/* Sparse matrix times point vector, on the handle of an Fr matrix as it stands:
 *     out[i] = sum over the kept entries k of row i of the handle of  coeff[k] * P[col[k]],   i < n_rows
 * a row without kept entries gives the group's zero.  With the transposed handle of a constraint matrix and P the
 * Lagrange form [L_i(tau)]G of a ceremony's powers (amdmsm_group_fft, inverse) this is a Groth16 query of a phase-2
 * setup, A_query[c] = sum over the entries (i, c) of A of A[i][c] * [L_i(tau)]G -- the map amdmsm_fr_matrix_apply runs
 * over Fr when the trapdoor is known.  DESIGN section 28.
 *   mat      any live handle of this context (amdmsm_fr_matrix_load or _load_transposed) of the curve `curve`; it keeps
 *            serving amdmsm_fr_matrix_apply*, before and after and on other streams, and amdmsm_fr_matrix_free waits for
 *            the applies of this entry too.  A handle loaded under AMDMSM_FR_MATRIX_NAIVE=1 has no resident form and is
 *            refused.
 *   chunk_entries  general-coefficient entries worked through at a time (each costs one ladder of amdmsm_scalar_mul_vec
 *            and its table in the workspace); 0 = as many as fit that entry's 1 GiB budget.  Chunks are cut between wave
 *            jobs, so a job with more general entries than this still runs whole.  The results do not depend on it,
 *            bit for bit.
 * amdmsm_group_matrix_apply_device: n_points >= n_cols compact affine records (amdmsm_import_bases_device) in, n_rows
 * records in opts->out_form (AMDMSM_OUT_LIBFF by default; AMDMSM_OUT_AFFINE is normalised in batch) out, both in HBM and
 * not overlapping; nothing at or beyond record n_rows is touched.  Enqueued on opts->stream (or the context's), not
 * synchronised.  Entries of coefficient 1 and r - 1 cost one mixed addition each.
 * amdmsm_group_matrix_apply: records, stride and base_form as for amdmsm_multi_exp, out_xyz n_rows packed records in host
 * memory; uploads, applies, downloads and synchronises.
 * Refused before anything is launched or written, in this order: AMDMSM_ERR_UNSUPPORTED for (MNT6, G2) or an unknown
 * curve or group (before the context is looked at); AMDMSM_ERR_BAD_ARG, with amdmsm_last_error naming the argument, for a
 * null context, a wrong opts->struct_size, a handle that is freed, foreign, of another curve or naive, n_points < n_cols,
 * a null pointer with work to do, a bad stride or alignment, an output overlapping the input; AMDMSM_ERR_TOO_LARGE for
 * n_points above 2^28.  A handle with 0 rows succeeds and writes nothing.
 * amdmsm_plan_group_matrix, read-only: out[0] / out[1] general / +-1 entries kept, out[2] wave jobs, out[3] partial sums,
 * out[4] chunks for this chunk_entries, out[5] workspace bytes, out[6] launches (AMDMSM_OUT_LIBFF), out[7] 0.
 * With timing enabled (amdmsm_get_timings): [0] import with upload (host entry), [1] the general pass -- gather, table,
 * ladder, normalisation -- [2] accumulation and combine, [3] normalisation / export of the output (host entry: with the
 * download), [AMDMSM_PH_TOTAL] the call. */
int amdmsm_group_matrix_apply_device(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, const void *d_points_affine,
                                     size_t n_points, void *d_out_xyz, size_t chunk_entries, const amdmsm_opts *opts);
int amdmsm_group_matrix_apply(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, const void *points_xyz,
                              size_t stride_bytes, int base_form, size_t n_points, void *out_xyz, size_t chunk_entries,
                              const amdmsm_opts *opts);
int amdmsm_plan_group_matrix(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, size_t chunk_entries, size_t out[8]);

/* Segmented MSM: m sums in one call, out[j] = sum of scalars[i] * base(i) over offsets[j] <= i < offsets[j + 1] -- the
 * shape of k proofs verified as a batch (sum of input_i * IC_i per proof), of row or column commitments, of the cross
 * terms of an inner-product argument.  A single MSM per segment would pay the fixed cost of its launch chain m times;
 * here a lane owns one (segment, 4-bit window) pair, adds the segment's terms from the table of amdmsm_scalar_mul_vec
 * without ever doubling, and the doublings are paid once per segment in a Horner chain.
 *   bases     as for amdmsm_multi_exp (records, stride, form).  Without flags n_bases == n_terms and term i uses base
 *             i; with AMDMSM_SEG_SHARED_BASES term i of segment j uses base i - offsets[j] (one query shared by all
 *             segments, its table built once), and n_bases is at least the longest segment
 *   scalars   n_terms Montgomery residues, or with opts->scalars_plain any integers of fr_bytes (k >= r means k mod r)
 *   offsets   m + 1 values in HOST memory (in the device entry too), non-decreasing, offsets[m] <= n_terms;
 *             offsets[0] may be above 0; terms outside every segment are ignored, an empty segment gives zero
 *   long_from segments of at least this many terms are run one after the other through the single-MSM route of
 *             amdmsm_msm_device instead; 0 = the library's default, SIZE_MAX = never
 *   out       m packed records in opts->out_form (AMDMSM_OUT_LIBFF by default; AMDMSM_OUT_AFFINE normalises the batch
 *             as amdmsm_batch_to_special does), written only when the call succeeds
 * AMDMSM_ERR_BAD_ARG, with amdmsm_last_error naming the segment, before anything is launched or written: a null
 * pointer with work to do, a bad stride, a decreasing offset, offsets[m] > n_terms, an unknown flag, n_bases != n_terms
 * without the flag, a segment longer than n_bases with it.  m = 0 succeeds and writes nothing.  The workspace follows
 * the 1 GiB rule of amdmsm_scalar_mul_vec, chunked by whole segments.  With timing enabled: [0] table, [1] digits,
 * [2] accumulation, [3] Horner -- of the first chunk -- [4] its normalisation and the chunks after it,
 * [AMDMSM_PH_TOTAL] the segment pass; a segment on the single-MSM route is a timed MSM of its own. */
#define AMDMSM_SEG_SHARED_BASES 1u
int amdmsm_multi_exp_segments(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                              int base_form, size_t n_bases, const void *scalars, size_t n_terms,
                              const uint64_t *offsets, size_t m, unsigned flags, size_t long_from, void *out,
                              const amdmsm_opts *opts);
/* the same on device-resident inputs: compact affine bases, m records written to d_out; enqueued on opts->stream (or the
 * context's), not synchronised */
int amdmsm_msm_device_segments(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, size_t n_bases,
                               const void *d_scalars, size_t n_terms, const uint64_t *offsets, size_t m,
                               unsigned flags, size_t long_from, void *d_out, const amdmsm_opts *opts);
/* terms a segmented MSM of this context works through at a time (whole segments; a longer segment is a chunk of its own),
 * 0 = as many as fit the workspace rule (the default) */
int amdmsm_set_segments_chunk_terms(amdmsm_ctx *ctx, size_t chunk_terms);

/* k (<= 8) multi_exp calls of the same group, length and base form as ONE batch: for a caller that has k base vectors
 * of ONE length with a scalar vector each, instead of k calls of multiexp.tcc:643-688.  (The four G1 MSMs of libsnark's
 * r1cs_gg_ppzksnark_prover -- A, B, L, H -- have different lengths and share the assignment as their scalar vector:
 * that call sequence is amdmsm_multi_exp_batch_items below.)  Same results as k amdmsm_multi_exp calls; the
 * latency-bound tails of the k MSMs run as one set of kernels (amdmsm_msm_device_batch).  Registered base vectors are
 * honoured per MSM. */
int amdmsm_multi_exp_batch(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *bases_xyz,
                           size_t base_stride_bytes, int base_form, const void *const *scalars, size_t n,
                           void *const *out_xyz, const amdmsm_opts *opts);

/* One MSM of a batch of MSMs of different lengths (amdmsm_multi_exp_batch_items / amdmsm_msm_device_batch_items).
 * Its scalars are a vector of its own, or are taken from ONE vector the whole batch shares: a contiguous slice of it
 * or the elements an index list names (libsnark's sparse_vector queries select the assignment's entries by index).
 * The selection happens on the device inside the digit pass; the shared vector crosses PCIe once per call. */
typedef struct amdmsm_batch_item {
    uint32_t struct_size;  /* = sizeof(amdmsm_batch_item) (AMDMSM_BATCH_ITEM_INIT); an unknown size is refused */
    const void *bases;     /* host entry: n libff (X, Y, Z) records (registered vectors are honoured);
                              device entry: n compact affine records in HBM */
    size_t n;              /* terms of this MSM; 0 gives the group's zero */
    const void *scalars;   /* this MSM's own n scalars, or NULL: take them from the shared vector */
    size_t shared_offset;  /* scalars == NULL, index == NULL: term i uses shared[shared_offset + i] */
    const uint32_t *index; /* scalars == NULL: term i uses shared[index[i]]; any order, repeats allowed */
    void *out_xyz;         /* one (X, Y, Z) record in opts->out_form */
} amdmsm_batch_item;
#define AMDMSM_BATCH_ITEM_INIT { (uint32_t)sizeof(amdmsm_batch_item) }

/* k (1 .. 8) multi_exp calls of one group and base form, each of its own length, as ONE batch: one window size for the
 * whole batch (chosen for the longest MSM), sort and accumulation MSM after MSM, the latency-bound tail once over the
 * windows of all of them.  Same results as k amdmsm_multi_exp calls on the selected scalars.  shared_scalars (shared_n
 * elements, may be NULL when every item brings its own) is uploaded once; own vectors and index lists per item.
 * Everything is validated before anything is launched -- k, struct_size, a slice past shared_n, an index >= shared_n,
 * scalars together with index, a missing shared vector, the stride rules of amdmsm_multi_exp: AMDMSM_ERR_BAD_ARG, the
 * outputs untouched.  opts apply to the whole batch; window_bits > 22 is AMDMSM_ERR_BAD_ARG, as for
 * amdmsm_multi_exp_batch.  A batch with sum n >= 2^30 or an item too long for one pass runs its MSMs one after the
 * other, their scalars gathered on the device.  No filter_one_zero statistics, one group per batch, one device. */
int amdmsm_multi_exp_batch_items(amdmsm_ctx *ctx, int curve, int group, int k, const amdmsm_batch_item *items,
                                 size_t base_stride_bytes, int base_form, const void *shared_scalars, size_t shared_n,
                                 const amdmsm_opts *opts);

/* ---- scalars known to be short ----
 * libff's multi_exp sizes its rounds by num_bits = max_i bi_exponents[i].num_bits() (multiexp.tcc:297-304, :577-586): a
 * vector of bytes or 32-bit words costs it an eighth of a vector of full-length scalars.  The entries below do the same:
 * the windows cover the scalars' bit length, and packed integers are read as they are -- n * width bytes cross PCIe and
 * pass through the digit kernel instead of n Fr records.  They return the group element amdmsm_multi_exp /
 * amdmsm_msm_device return for the same values widened to Fr.
 *   kind  AMDMSM_SCALAR_FR: Fr records as everywhere else (Montgomery, or plain with opts->scalars_plain).
 *         AMDMSM_SCALAR_U8 / U16 / U32 / U64: packed little-endian unsigned integers; the pointer needs the element's
 *         own alignment only, and opts->scalars_plain is ignored.
 *   bits  0: the kind's full width (Fr::num_bits, or 8 * width) -- the type bounds the value, nothing is tested;
 *         N > 0: the caller's promise that every scalar is < 2^N.  It is tested on the device; a scalar that breaks it
 *           makes the call return AMDMSM_ERR_BAD_ARG with the output untouched.  The call synchronises to learn that.
 *         -1: the bit length is measured on the device (amdmsm_scalar_bits_device) before the plan is made: the call
 *           reads 4 bytes back first and is therefore synchronous; all scalars zero gives the group's zero.
 * num_windows = (bits + 2 + c - 1) / c; c comes from the cost model with bits in place of Fr::num_bits and is never
 * larger than bits + 2.  The endomorphism split is used only where amdmsm_plan_ex would use it and bits exceeds the
 * split's own bound (amdmsm_endomorphism_info); bits >= Fr::num_bits is the ordinary plan.  amdmsm_plan_short tells
 * (scalar_bits = 0: full width).  opts->window_bits > 22 is AMDMSM_ERR_BAD_ARG, as for the batch calls.  Everything is
 * validated before anything is launched.  Signed integers, batches, the precomputed-table and streaming paths and
 * several GPUs are not covered. */
enum { AMDMSM_SCALAR_FR = 0, AMDMSM_SCALAR_U8 = 1, AMDMSM_SCALAR_U16 = 2, AMDMSM_SCALAR_U32 = 4, AMDMSM_SCALAR_U64 = 8 };
typedef struct amdmsm_scalar_desc {
    uint32_t struct_size; /* = sizeof(amdmsm_scalar_desc) (AMDMSM_SCALAR_DESC_INIT); an unknown size is refused */
    int kind;             /* AMDMSM_SCALAR_* */
    int bits;             /* 0, N > 0 or -1, see above */
} amdmsm_scalar_desc;
#define AMDMSM_SCALAR_DESC_INIT { (uint32_t)sizeof(amdmsm_scalar_desc) }
int amdmsm_plan_short(int curve, int group, size_t n, int window_bits, int endomorphism, int scalar_bits, int *c,
                      int *num_windows, uint32_t *num_buckets, size_t *workspace_bytes, int *endomorphism_used);
/* *bits = bit length of the longest of the n device-resident scalars (0: all zero); desc->bits is not read.
 * Runs on the context stream and synchronises it. */
int amdmsm_scalar_bits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n,
                              const amdmsm_scalar_desc *desc, int scalars_plain, int *bits);
/* amdmsm_multi_exp on short scalars: registered bases and AMDMSM_BASE_CACHE_MB are honoured in the same way, inputs above
 * AMDMSM_MAX_RANGE_POINTS run as ranges with one bit length for all of them */
int amdmsm_multi_exp_short(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                           int base_form, const void *scalars, const amdmsm_scalar_desc *desc, size_t n, void *out_xyz,
                           const amdmsm_opts *opts);
/* amdmsm_msm_device on short scalars.  Asynchronous like amdmsm_msm_device only with bits = 0; with a promise
 * (synchronises to read the flag, the result is written after that) or bits = -1 (synchronises to read the measured
 * length) the call returns when the result is in d_out_xyz. */
int amdmsm_msm_device_short(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, const void *d_scalars,
                            const amdmsm_scalar_desc *desc, size_t n, void *d_out_xyz, const amdmsm_opts *opts);

/* Resident base vectors.  A prover calls multi_exp with the same base vector (its proving key,
 * libsnark r1cs_gg_ppzksnark_proving_key) proof after proof; the reference re-reads it from host
 * memory every time (multiexp.tcc:643-688 takes const iterators).  amdmsm_register_bases imports
 * the vector once (libff records -> compact affine in HBM, Montgomery's trick for normal-form
 * bases) and from then on every amdmsm_multi_exp[_multi|_filter_one_zero] call whose base range
 * lies inside [bases_xyz, bases_xyz + n*stride) with the same stride and form reads the resident
 * copy: only the scalars cross PCIe.  The caller promises not to modify a registered vector
 * without amdmsm_invalidate_bases (any registration overlapping [host_ptr, host_ptr + bytes);
 * NULL = all) or amdmsm_unregister_bases.  AMDMSM_BASE_CACHE_MB=<MiB> in the environment makes
 * the host entry points register what they see automatically (LRU within the cap); off by default
 * because of that promise.  A registered vector also keeps the (beta x, y) records of the
 * endomorphism split (amdmsm_opts.endomorphism) once a call has used them: twice the compact
 * affine bytes in HBM, and no per-call kernel for them. */
int amdmsm_register_bases(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz,
                          size_t base_stride_bytes, int base_form, size_t n, uint64_t *handle);
int amdmsm_unregister_bases(amdmsm_ctx *ctx, uint64_t handle);
int amdmsm_invalidate_bases(amdmsm_ctx *ctx, const void *host_ptr, size_t bytes);

/* multi_exp over several GPUs of one node from ONE process (what a C++ host such as libsnark
 * has): libff's own range split (multiexp.tcc:655-687, `one = total / chunks`, the last range
 * takes the remainder) with chunk = device.  ctxs[k] (one context per device, or several
 * contexts on one device) reduces its range on its own device from its own host thread; the
 * ndev partial points travel to ctxs[0]'s device (hipMemcpyPeerAsync over xGMI) and are summed
 * there (multiexp.tcc:681-687).  Resident bases are honoured per context: register each range
 * with its context. */
int amdmsm_multi_exp_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group,
                           const void *bases_xyz, size_t base_stride_bytes, int base_form,
                           const void *scalars, size_t n, void *out_xyz, const amdmsm_opts *opts);
/* multi_exp_filter_one_zero (multiexp.tcc:690-757) over the same device split: every device classifies the
 * scalars of its own range, the three counts are added up (stats may be NULL = amdmsm_multi_exp_multi) */
int amdmsm_multi_exp_filter_one_zero_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group,
                                           const void *bases_xyz, size_t base_stride_bytes, int base_form,
                                           const void *scalars, size_t n, void *out_xyz,
                                           const amdmsm_opts *opts, size_t stats[3]);

/* Streaming MSM: bases are pulled through `read` in libff's on-disk format -- binary,
 * Montgomery form, uncompressed, i.e. consecutive group_write<encoding_binary, form_montgomery,
 * compression_off> records (curve_serialization.tcc:78-101; what profile_multiexp.cpp:100-150
 * writes) -- chunk by chunk, so they never need to be resident at once.  Replaces
 * multi_exp_stream<form_montgomery, compression_off, G, Fr> (multiexp_stream.hpp:25-33,
 * multiexp_stream.tcc:164-191).  `read` returns the number of bytes delivered (0 = end).
 * chunk_points = 0 picks 2^20. */
typedef size_t (*amdmsm_read_fn)(void *read_ctx, void *dst, size_t bytes);
int amdmsm_multi_exp_stream(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read, void *read_ctx,
                            const void *scalars, size_t n, size_t chunk_points, void *out_xyz,
                            const amdmsm_opts *opts);
int amdmsm_multi_exp_stream_file(amdmsm_ctx *ctx, int curve, int group, const char *path,
                                 size_t offset_bytes, const void *scalars, size_t n,
                                 size_t chunk_points, void *out_xyz, const amdmsm_opts *opts);

/* The same with compressed records -- multi_exp_stream<form_montgomery, compression_on, G, Fr>:
 * group_write<encoding_binary, form_montgomery, compression_on> (curve_serialization.tcc:103-133)
 * stores X only (for Fq2: c0 then c1), big-endian Montgomery limbs, with two flags in the top bits
 * of the first byte (bit 0: lowest bit of Y.c0's Montgomery representation, bit 1: zero); the
 * device recovers Y = sqrt(X^3 + b) (curve_utils.tcc:34-47; Tonelli-Shanks for bls12_377's Fq,
 * a^((q+1)/4) otherwise; Fq2 by the norm method) and fixes its sign from the flag.  An X that is
 * not the abscissa of a curve point makes the call fail with AMDMSM_ERR_BAD_ARG (the reference's
 * sqrt does not terminate on such input). */
int amdmsm_multi_exp_stream_compressed(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read,
                                       void *read_ctx, const void *scalars, size_t n,
                                       size_t chunk_points, void *out_xyz, const amdmsm_opts *opts);
int amdmsm_multi_exp_stream_compressed_file(amdmsm_ctx *ctx, int curve, int group, const char *path,
                                            size_t offset_bytes, const void *scalars, size_t n,
                                            size_t chunk_points, void *out_xyz,
                                            const amdmsm_opts *opts);

/* Streaming MSM over precomputed multiples.  Replaces multi_exp_stream_with_precompute<
 * form_montgomery, compression_off, G, Fr> (multiexp_stream.hpp:29-42, multiexp_stream.tcc:
 * 193-223): the stream holds, for every base P, the amdmsm_precompute_num_digits(curve, c)
 * records P, [2^c]P, [2^2c]P, ... (what create_precompute_file_for_config writes,
 * profile_multiexp.cpp:120-150); digit j of a scalar selects the bucket for record j, all in
 * ONE set of 2^(c-1) buckets, and no doublings are needed.  As in the reference, a carry out of
 * the last digit is dropped.  chunk_points = 0 picks about 2^20 records per chunk. */
size_t amdmsm_precompute_num_digits(int curve, size_t c);   /* (Fr::num_bits + c - 1) / c */
int amdmsm_multi_exp_stream_with_precompute(amdmsm_ctx *ctx, int curve, int group,
                                            amdmsm_read_fn read, void *read_ctx,
                                            const void *scalars, size_t n, size_t precompute_c,
                                            size_t chunk_points, void *out_xyz,
                                            const amdmsm_opts *opts);
int amdmsm_multi_exp_stream_with_precompute_file(amdmsm_ctx *ctx, int curve, int group,
                                                 const char *path, size_t offset_bytes,
                                                 const void *scalars, size_t n,
                                                 size_t precompute_c, size_t chunk_points,
                                                 void *out_xyz, const amdmsm_opts *opts);

/* Fixed-base batch exponentiation: out[i] = scalars[i] * g (or (coeff * scalars[i]) * g when
 * coeff != NULL), i < n, through a window table built on the device.  Replaces
 * get_window_table + batch_exp / batch_exp_with_coeff (multiexp.hpp:99-134,
 * multiexp.tcc:809-947); `scalar_size` and `window` have the reference's meaning
 * (FieldT::size_in_bits(), get_exp_window_size).  out: n packed (X, Y, Z) records. */
int amdmsm_batch_exp(amdmsm_ctx *ctx, int curve, int group, size_t scalar_size, size_t window,
                     const void *g_xyz, const void *scalars, size_t n, const void *coeff,
                     int scalars_plain, void *out_xyz);
/* device times (ms) of the context's last amdmsm_batch_exp: [0] inputs host -> device, [1] window table
 * (get_window_table, multiexp.tcc:809-846; 0 when the table of the previous call -- same group, scalar_size,
 * window and g -- was still resident), [2] the exponentiations (batch_exp's loop, :874-912), [3] results back */
int amdmsm_get_batch_exp_timings(amdmsm_ctx *ctx, float ms[4]);

/* amdmsm_batch_exp on device-resident scalars, the results left in HBM: d_out_xyz[i] = d_scalars[i] * g (or (coeff *
 * d_scalars[i]) * g), what a key generator calls on the Fr vectors amdmsm_fr_lincomb_device left on the device.
 * scalar_size, window, g_xyz (host) and coeff (host Fr record or NULL) mean what they mean in amdmsm_batch_exp;
 * opts->scalars_plain speaks of d_scalars and of coeff.  opts->out_form: AMDMSM_OUT_LIBFF (opts == NULL) gives the
 * records amdmsm_batch_exp writes, word for word; AMDMSM_OUT_AFFINE special form, by the batch normalisation of
 * amdmsm_scalar_mul_vec_device; AMDMSM_OUT_JACOBIAN is refused.  amdmsm_import_bases_device (form normal, or special
 * after AMDMSM_OUT_AFFINE) turns the results into compact affine records for the MSM entries and the writers below.
 * Enqueued on opts->stream (or the context's) and not synchronised; g_xyz and coeff are consumed before the call
 * returns.  n = 0 succeeds, writes nothing and still builds or keeps the table.
 * The context's resident window table is shared with amdmsm_batch_exp under the same rule -- same curve, group,
 * scalar_size, window and g: a table built by either entry serves the other, and a call on another stream than the
 * one that built or last read it waits for that call on the device (an event, as for a workspace slot).  One table.
 * Refused before anything is launched or written: AMDMSM_ERR_UNSUPPORTED for (MNT6, G2), before the context is looked
 * at; AMDMSM_ERR_BAD_ARG for window outside 1..22, scalar_size outside 1..8 * fr_bytes, a null g, a wrong
 * opts->struct_size, and with n > 0 a null device pointer, d_scalars off 16 bytes (8 for the 10-word fields) or
 * d_out_xyz off the record alignment, d_out_xyz overlapping d_scalars.
 * amdmsm_get_batch_exp_timings after this entry waits for the call: [0] upload of g / coeff, [1] table (0 when
 * reused), [2] exponentiations, [3] normalisation (0 for AMDMSM_OUT_LIBFF).  The normalisation of AMDMSM_OUT_AFFINE
 * takes a workspace slot, as amdmsm_scalar_mul_vec_device does: on a context with amdmsm_set_timing on it takes a timing
 * ticket too, so amdmsm_get_timings, amdmsm_last_timing_ticket and amdmsm_last_slot then speak of this call and no
 * longer of the MSM before it (all of the slot's time stands under its last phase). */
int amdmsm_batch_exp_device(amdmsm_ctx *ctx, int curve, int group, size_t scalar_size, size_t window,
                            const void *g_xyz /* host */, const void *d_scalars, size_t n,
                            const void *coeff /* host Fr record or NULL */, void *d_out_xyz,
                            const amdmsm_opts *opts);

/* ---- device-resident entry points (all pointers are HBM addresses) ---- */
int amdmsm_import_bases_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_xyz,
                               size_t stride_bytes, int base_form, size_t n, void *d_dst_affine,
                               void *stream);
int amdmsm_export_affine_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_affine,
                                size_t n, void *d_dst_xyz, void *stream);
/* group_read<encoding_binary, form_montgomery, compression_{off,on}> over n on-disk records that
 * are already in HBM -> n compact affine points (curve_serialization.tcc:78-101, 134-166);
 * *status != 0: some compressed X is not on the curve.  Synchronises. */
int amdmsm_disk_decode_device(amdmsm_ctx *ctx, int curve, int group, const void *d_records, size_t n,
                              int compressed, void *d_dst_affine, unsigned *status);
/* The inverse: group_write<encoding_binary, form_montgomery, compression_{off,on}> (curve_serialization.tcc:78-133) of
 * n compact affine points in HBM -> n on-disk records in HBM, 2 * coordinate bytes each (compressed: one coordinate).
 * Uncompressed: X || Y, every Fq component the Montgomery residue with its bytes reversed, Fq2 as c0 then c1; zero is
 * written (0, one), what the reference writes after to_affine_coordinates.  Compressed (the a = 0 curves;
 * AMDMSM_ERR_UNSUPPORTED for MNT4 / MNT6): X with two flags in the top bits of the first byte -- bit 0 the low bit of
 * Y's (Y.c0's) Montgomery representation, bit 1 zero, which is written as X = 0 with that flag alone.
 * Enqueued on `stream` (NULL: the context's) and not synchronised; n = 0 succeeds.  AMDMSM_ERR_BAD_ARG for a null or
 * misaligned vector with n > 0 (the record alignment: 16 bytes, 8 for the 10-word fields) and for d_records overlapping
 * the source. */
int amdmsm_disk_encode_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_affine, size_t n,
                              int compressed, void *d_records, void *stream);
/* The same records, written out: n compact affine points in HBM leave through `write` (or into a file) in the format
 * amdmsm_multi_exp_stream[_compressed][_file] and -- for a table of amdmsm_precompute_bases_device --
 * amdmsm_multi_exp_stream_with_precompute[_file] read.  chunk_points records at a time (0: 2^20, the readers' default):
 * chunk k is encoded on the device and copied into one of two pinned staging buffers while chunk k - 1 is handed to
 * `write`, which sees the records in order, one call per chunk, and returns the bytes it took.  A callback that takes
 * fewer bytes than offered ends the call with AMDMSM_ERR_BAD_ARG ("record stream ended early"); the context stays
 * usable.  The points have to be complete on the context's stream; the call returns when everything is written.
 * amdmsm_write_points_file opens `path` without truncating it (creating it where absent) and writes from offset_bytes
 * on: the bytes in front and those behind the records are left as they are.  A file that cannot be opened or written
 * is AMDMSM_ERR_BAD_ARG ("cannot open <path>", "cannot write <path>"), as for the _file readers.
 * amdmsm_plan_write_points (no context): out[0] = chunks of such a call, and for chunk k below that number out[1] =
 * its first record, out[2] = its records, out[3] = its staging buffer. */
typedef size_t (*amdmsm_write_fn)(void *write_ctx, const void *src, size_t bytes); /* returns bytes taken */
int amdmsm_write_points_stream(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n,
                               int compressed, amdmsm_write_fn write, void *write_ctx, size_t chunk_points);
int amdmsm_write_points_file(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n,
                             int compressed, const char *path, size_t offset_bytes, size_t chunk_points);
int amdmsm_plan_write_points(size_t n, size_t chunk_points, size_t k, size_t out[4]);
int amdmsm_msm_device(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine,
                      const void *d_scalars, size_t n, void *d_out_xyz, const amdmsm_opts *opts);
/* k (<= 8) MSMs of the same group and length in one call: d_bases_affine[j] / d_scalars[j] / d_out_xyz[j] as for
 * amdmsm_msm_device, all results in opts->out_form.  The reference has no such entry -- a prover calls multi_exp
 * (multiexp.tcc:643-688) once per query vector of its proving key -- but those calls are independent, and on the device
 * their latency-bound tails (bucket fix-up, reduction, final Horner) then run once over the windows of all k MSMs
 * instead of once per MSM.  Same results as k single calls. */
int amdmsm_msm_device_batch(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *d_bases_affine,
                            const void *const *d_scalars, size_t n, void *const *d_out_xyz, const amdmsm_opts *opts);
/* amdmsm_multi_exp_batch_items on device-resident inputs: every pointer inside items[] (the array itself is in host
 * memory) and d_shared_scalars are HBM addresses, bases are compact affine.  Slices are checked on the host.  Index
 * lists cannot be: the digit pass never dereferences an index >= shared_n -- it takes scalar 0 for it and raises a flag
 * -- and a call that has index lists synchronises the stream to read that flag: AMDMSM_ERR_BAD_ARG names the item, the
 * outputs of the batch are then meaningless.  Without index lists the call is asynchronous like amdmsm_msm_device. */
int amdmsm_msm_device_batch_items(amdmsm_ctx *ctx, int curve, int group, int k, const amdmsm_batch_item *items,
                                  const void *d_shared_scalars, size_t shared_n, const amdmsm_opts *opts);
/* The same with the table resident in HBM (288 GB hold [2^(jc)]P for 2^26 alt_bn128 G1 bases):
 * amdmsm_precompute_bases_device fills d_table[i * num_digits + j] = [2^(j*c)] P_i (compact
 * affine, n * num_digits records) from compact affine bases -- the device-side
 * create_precompute_file_for_config -- and amdmsm_msm_precomputed_device is
 * multi_exp_precompute_from_fifo (multiexp_stream.tcc:124-162) on it.  num_digits =
 * amdmsm_precompute_num_digits() reproduces the reference; one more digit where
 * c divides Fr::num_bits keeps the final carry.  Inputs with n * num_digits >= 2^31 are split
 * into ranges of points internally. */
int amdmsm_precompute_bases_device(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine,
                                   size_t n, size_t c, size_t num_digits, void *d_table, void *stream);
int amdmsm_msm_precomputed_device(amdmsm_ctx *ctx, int curve, int group, const void *d_table,
                                  const void *d_scalars, size_t n, size_t c, size_t num_digits,
                                  void *d_out_xyz, const amdmsm_opts *opts);
/* the device-resident form of amdmsm_multi_exp_multi: d_bases_affine[k] / d_scalars[k] / counts[k]
 * live on ctxs[k]'s device; the result is written to d_out_xyz_dev0 on ctxs[0]'s device
 * (opts->stream, a stream of ctxs[0]'s device: inputs produced on it are ordered before every range, and
 * the final sum runs on it; the call returns after that sum has completed).
 * Any entry point given more than 2^28 points (AMDMSM_MAX_RANGE_POINTS) runs them as contiguous ranges
 * whose partial results are summed -- the reference's chunk loop, multiexp.tcc:655-687. */
int amdmsm_msm_device_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group,
                            const void *const *d_bases_affine, const void *const *d_scalars,
                            const size_t *counts, void *d_out_xyz_dev0, const amdmsm_opts *opts);
/* sum of k engine-Jacobian partial results (multi-GPU / chunk combination, multiexp.tcc:681-687) */
int amdmsm_sum_points_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_jacobian,
                             int k, int out_form, void *d_out_xyz, void *stream);
/* synthetic benchmark input: dst[i] = (first + i + 1) * G::one(), compact affine */
int amdmsm_gen_bases_seq_device(amdmsm_ctx *ctx, int curve, int group, uint64_t first, size_t n,
                                void *d_dst_affine, void *stream);

/* ---- MSMs in flight ----
 * depth = number of workspace slots (1..4, default 1) taken round-robin by consecutive
 * amdmsm_msm_device calls.  With depth > 1, calls issued on DIFFERENT streams may overlap on
 * the device (a prover's back-to-back MSMs: the few-wave tail of one under the bulk kernels
 * of the next); a slot is reused only after its previous call has completed. */
int amdmsm_set_pipeline_depth(amdmsm_ctx *ctx, int depth);
/* slot used by the most recent amdmsm_msm_device call */
int amdmsm_last_slot(amdmsm_ctx *ctx);

/* ---- per-phase device timing (hipEvents on the launch stream) ---- */
int amdmsm_set_timing(amdmsm_ctx *ctx, int enable);
/* milliseconds of the most recent amdmsm_msm_device call; waits for that call */
int amdmsm_get_timings(amdmsm_ctx *ctx, float ms[AMDMSM_MAX_PHASES]);
/* every timed call also gets a ticket (0, 1, 2, ...); the phase times of the last 64 tickets stay
 * readable, so a caller can enqueue MSM after MSM on one stream without synchronising in between
 * and collect all the timings afterwards.  amdmsm_last_timing_ticket: ticket of the most recent
 * timed call (-1: none). */
long long amdmsm_last_timing_ticket(amdmsm_ctx *ctx);
int amdmsm_get_timings_by_ticket(amdmsm_ctx *ctx, long long ticket, float ms[AMDMSM_MAX_PHASES]);
/* same for the call that last used workspace slot `slot` */
int amdmsm_get_slot_timings(amdmsm_ctx *ctx, int slot, float ms[AMDMSM_MAX_PHASES]);

/* ---- parity-test hooks for the primitives (device pointers) ---- */
int amdmsm_field_op_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_a,
                           const void *d_b, void *d_out, size_t n);
int amdmsm_group_op_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_a,
                           const void *d_b, void *d_out, size_t n, int out_form);
/* One coordinate-field function per element, on the element type of the cold kernels (impl 0) or the
 * fully inlined one (impl 1).  Operands and result are arrays of n elements of el_words 32-bit words,
 * taken and stored as they are; d_b, d_c, d_d are null where the op takes fewer operands.  d_flag (may be
 * null): one word per element, the boolean the op returns, else 0.
 * Canonical ops, operands in [0, p) per component: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 inverse, 6 double,
 * 7 conditional negate (where the low bit of b's first word is set), 8 half, 9 to Montgomery form,
 * 10 from Montgomery form, 11 square root (flag: a is a square; either root).
 * Almost-reduced ops, operands in [0, 2p) per component, results below 2p: 16 mul, 17 sqr, 18 sub,
 * 19 add, 20 neg, 21 a b - c d, 22 is zero (flag), 23 canonical representative. */
int amdmsm_field_probe_device(amdmsm_ctx *ctx, int curve, int group, int impl, int op, const void *d_a,
                              const void *d_b, const void *d_c, const void *d_d, void *d_out,
                              uint32_t *d_flag, size_t n);
/* One extended-Jacobian (X, Y, ZZ, ZZZ) function per lane, impl as above: 0 mixed addition on
 * almost-reduced coordinates, 1 mixed addition, 2 addition, 3 doubling, 4 doubling of an affine point,
 * 5 conversion to Jacobian (X, Y, Z, then zeros).  d_acc and d_out: n records of 4 * el_words words;
 * d_pt: n compact affine records (ops 0, 1, 4) or n more (X, Y, ZZ, ZZZ) records (op 2), else null. */
int amdmsm_xyzz_probe_device(amdmsm_ctx *ctx, int curve, int group, int impl, int op, const void *d_acc,
                             const void *d_pt, void *d_out, size_t n);
/* The reduced-radix layer (signed limbs of B = 28 / 29 bits, L per Fq component; rho = 2^(B L) = 2^D 2^(32 fq_words))
 * that the bucket accumulation of the pairing-friendly groups runs on: one function per element on RAW limbs, taken and
 * stored as they are.  AMDMSM_ERR_UNSUPPORTED, with amdmsm_last_error naming the group and nothing written, for the
 * MNT groups, which do not use it.  Arrays hold one row per Fq component: n rows for an Fq group, 2 n for an Fq2 group
 * (element i = rows 2 i and 2 i + 1 = c0, c1).  d_a .. d_d: rows of L int32 limbs (null where the op takes fewer);
 * d_w: rows of fq_words words (ops that start from words); d_out: rows of L limbs; d_outw: rows of fq_words words, zero
 * where the op yields none; d_flag: one word per ELEMENT (an Fq2 element: the test holds in both components).
 * Products: 0 a b, 1 a b + c d, 2 a^2 -- each per component -- 3 element product, 4 element square, 5 element a b - c d
 * (Fq2: fused over the pair), 6 a 2^(32 fq_words) / rho, 7 a 2^(32 fq_words - D) / rho, 8 words -> limbs with the factor
 * rho, 9 / 10 export of a component with the factor rho / rho 2^D to canonical words (d_outw).
 * Others: 16 one parallel carry step, 17 full carry propagation, 18 k a and a carry step (k = 2, 3, 4), 19 negation of
 * the elements of odd index, 20 / 21 limbs of the words / of the words shifted by D, 22 the words 2^D less a multiple of
 * p (first point, reduced; AMDMSM_ERR_UNSUPPORTED for bw6_761, whose table of 2^16 multiples is not built), 23 the first-point coordinate of the group (22 or 21), 24 canonical limbs -> words (d_outw),
 * 25 a product's output in (-p, 2p) -> [0, p), 26 flag: a = 0 mod p exactly, 27 / 28 flag: the one-limb filter for
 * |j| < 2^D + 64 / < 64 (necessary for a = j p, not sufficient), 29 / 30 the constants 2^(B L), 2^(B L + D) mod p. */
int amdmsm_rr_probe_device(amdmsm_ctx *ctx, int curve, int group, int op, int k, const void *d_a, const void *d_b,
                           const void *d_c, const void *d_d, const void *d_w, void *d_out, void *d_outw,
                           uint32_t *d_flag, size_t n);
/* One step of one reduced-radix point function per element.  d_acc, d_sec, d_out: rows of 4 L limbs (X, Y, ZZ, ZZZ as a
 * lane of the accumulation holds them; the Jacobian ops: X, Y, Z, 0); d_pt: rows of 2 fq_words words, an affine point in
 * canonical Montgomery words, (0, 0) = infinity; d_fin (null: zeros) / d_fout: one word per element -- in: bit 0 the
 * accumulator is infinity, bit 1 the second operand is, bit 2 subtract the point; out: bit 0 the result is infinity,
 * bit 1 the answer of op 18.  d_outw: rows of 4 fq_words words, the result exported to canonical words as the readers of
 * a bucket record do it (zeros for infinity).
 * 0 mixed addition acc += pt, 1 first point of a bucket, 2 ZZ / ZZZ from the factor rho 2^D to rho, 3 / 4 the
 * accumulator unchanged, exported as a bucket record (ZZ, ZZZ with rho 2^D) / as a sum (rho), 8 doubling and 9 general
 * addition acc += sec on the factor rho, 16 Jacobian doubling, 17 Jacobian mixed addition of (sec.X, sec.Y), 18 Jacobian
 * infinity test. */
int amdmsm_xyzz_rr_probe_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_acc, const void *d_sec,
                                const void *d_pt, const uint32_t *d_fin, void *d_out, void *d_outw, uint32_t *d_fout,
                                size_t n);
int amdmsm_digits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n,
                         int scalars_plain, int c, int num_windows, int32_t *d_out);
/* throughput probes (2*iters dependent Fq products / iters mixed additions per lane);
 * *ms receives the kernel time from HIP events on the context stream */
/* endomorphism split (amdmsm_opts.endomorphism): lambda (plain integer, sizeof(Fr) bytes) with
   phi(P) = [lambda]P on the order-r subgroup, ceil(1000 log2) of the bound on |k1|, |k2|, and whether the
   whole curve group has order r.  The digits hook returns the signed digits of both halves,
   d_out[(2 i + half) * num_windows + w], so that sum_w d 2^(c w) over half 0 plus lambda times the same over
   half 1 is scalar i (mod r). */
int amdmsm_endomorphism_info(int curve, int group, void *lambda_plain, int *bound_log2_x1000, int *prime_order);
int amdmsm_endomorphism_digits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n,
                                      int scalars_plain, int c, int num_windows, int32_t *d_out);
int amdmsm_mul_bench_device(amdmsm_ctx *ctx, int curve, int group, void *d_inout, size_t nthreads,
                            int iters, int inline_variant, float *ms);
int amdmsm_madd_bench_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine,
                             void *d_out_xyz, size_t nthreads, int iters, int inline_variant, float *ms);

/* thin hipMalloc / hipMemcpy wrappers so non-HIP hosts (ctypes, cgo, JNI) can stage buffers */
int amdmsm_malloc(amdmsm_ctx *ctx, size_t bytes, void **d_ptr);
int amdmsm_free(amdmsm_ctx *ctx, void *d_ptr);
int amdmsm_memcpy_h2d(amdmsm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int amdmsm_memcpy_d2h(amdmsm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int amdmsm_synchronize(amdmsm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* AMDMSM_H */
