// Host-side table of kernel launchers for one (curve, group) pair.  One
// translation unit (msm_group.hip compiled with -DAMDMSM_GROUP=<traits>) fills one
// table; the engine (engine.cpp) is written against this table only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "fr_matrix_layout.h"

namespace amdmsm {

// output coordinate conventions for the final kernels
enum out_form : int {
    OUT_JACOBIAN = 0,   // engine-internal Jacobian (X, Y, Z); used for partial results
    OUT_LIBFF = 1,      // libff's in-memory coordinate system for the group (projective for bw6_761)
    OUT_AFFINE = 2,     // libff "special" form: (x, y, 1) or zero = (0, 1, 0)
};

// Geometry of the two-level bucket sort, shared by the launchers and the workspace planner.
struct sort_geom {
    int hb;               // coarse bits: bucket index = (coarse << fb) | fine
    int fb;
    uint32_t chunk_cap;   // entries per LDS chunk of the fine pass
    uint32_t big_thresh;  // a coarse bin above this many entries is sorted by many workgroups
    uint32_t big_cap;     // most such bins one call can hold (bound: total entries / big_thresh)
    size_t big_words;     // words of scratch for them: header + list + per-bin cursors
};
// The most coarse bits a plan takes, and with them the words of one window's coarse counters (2^hb bins and their total)
// and coarse-pass cursors (2^hb): the workspace holds both at this size whatever hb a call's length gives.
constexpr int SORT_HB_MAX = 10;
constexpr size_t SORT_COARSE_WORDS = ((size_t)1 << SORT_HB_MAX) + 1, SORT_CURSOR_WORDS = (size_t)1 << SORT_HB_MAX;
inline sort_geom sort_geometry(size_t n, int c, int W) {
    sort_geom g;
    // coarse / fine split of the c-1 bucket-index bits: about half each, at most 10 coarse and 11
    // fine bits (LDS tables of the two passes).  Measured (profiles/r02_sort_hb_sweep.txt): with
    // c = 16, 8 coarse bits beat 10 at every size from 2^16 to 2^23 (2^20: 0.27 vs 0.29 ms,
    // 2^16: 0.07 vs 0.09); around 2^20 points 7 is better still (0.24 ms).  AMDMSM_SORT_HB overrides.
    static const int hb_env = getenv("AMDMSM_SORT_HB") ? atoi(getenv("AMDMSM_SORT_HB")) : 0;
    g.hb = c / 2 < SORT_HB_MAX ? c / 2 : SORT_HB_MAX;
    if (c == 16 && n >= ((size_t)3 << 18) && n < ((size_t)3 << 19)) g.hb = 7;
    if (hb_env > 0) g.hb = hb_env;
    if (g.hb > c - 1) g.hb = c - 1;
    if (g.hb < 1) g.hb = 1;
    if (c - 1 - g.hb > 11) g.hb = c - 1 - 11;   // the fine pass handles at most 11 bits
    g.fb = c - 1 - g.hb;
    // The fine pass sorts a bin of up to chunk_cap entries in one piece and a longer one chunk by chunk; its LDS is
    // 6 bytes per entry of chunk_cap, and two of its 1024-thread workgroups share a CU up to about 13000.  So the cap
    // is the expected bin length mu = n / 2^hb plus a margin, not the next power of two above 2 mu: mu / 8 + 256 is at
    // least 8 standard deviations (sqrt(mu)) of a bin of a uniformly random input for every mu <= 16384, rounded up to
    // a multiple of 1024 (2^20 points, split: mu = 8192, cap 10240 = mu + 22 sigma).  1K .. 16K entries.
    static const uint32_t chunk_max = getenv("AMDMSM_SORT_CHUNK_MAX") ? (uint32_t)atoi(getenv("AMDMSM_SORT_CHUNK_MAX")) : 16384u;
    {
        const size_t mu = n >> g.hb;
        const size_t want = (mu + mu / 8 + 256 + 1023) / 1024 * 1024;
        g.chunk_cap = (uint32_t)(want < 1024 ? 1024 : want > chunk_max ? chunk_max : want);
    }
    g.big_thresh = 16 * g.chunk_cap;
    g.big_cap = (uint32_t)((size_t)W * n / g.big_thresh + 1);
    g.big_words = 4 + (size_t)g.big_cap * 4 + ((size_t)g.big_cap << g.fb);
    return g;
}

// Grid of the digit pass (k_sort_digits and its siblings).  The work items -- scalars, or 16-byte vectors of packed
// integers -- are cut into blocks of `block` consecutive items, thread t of a workgroup takes item block_index * block + t,
// and workgroup g of `grid` walks blocks g, g + grid, g + 2 grid, ...  It keeps ONE histogram in LDS over all of them and
// merges it into the global counters once, so a call costs grid * (counters per workgroup) global atomics whatever its
// length; wgs_max = the workgroups the device holds at once (or AMDMSM_SORT_DIGIT_WGS), so no workgroup waits for a CU.
// block is the workgroup size SORT_DIGIT_TPB; only where the items do not fill wgs_max such blocks is it halved, down to
// block_min (packed integers: a few thousand items are a large input).
constexpr uint32_t SORT_DIGIT_TPB = 1024;   // threads of a digit-pass workgroup (msm_group.hip SORT_TPB is this value)
struct digit_grid {
    uint32_t block;   // items per block, a power of two <= SORT_DIGIT_TPB
    size_t blocks;    // ceil(items / block)
    uint32_t grid;    // workgroups launched: min(blocks, wgs_max), 0 for no items
};
// wgs_max = 0: the resident count is not known (a failed query).  Then the grid is the one the pass had before it walked
// blocks -- 1024 workgroups, from 8192 blocks up one workgroup per 8 blocks -- which is right on any device.
inline digit_grid sort_digit_grid(size_t items, uint32_t block_min, uint32_t wgs_max) {
    digit_grid g;
    const uint32_t tpb = SORT_DIGIT_TPB;
    if (wgs_max < 1) {
        const size_t b = (items + tpb - 1) / tpb;
        wgs_max = (uint32_t)(b / 8 > 1024 ? (b + 7) / 8 : 1024);
    }
    if (block_min < 1 || block_min > tpb) block_min = tpb;
    g.block = tpb;
    while (g.block > block_min && (items + g.block - 1) / g.block < wgs_max) g.block >>= 1;
    g.blocks = (items + g.block - 1) / g.block;
    g.grid = (uint32_t)(g.blocks < wgs_max ? g.blocks : wgs_max);
    return g;
}

// The top window is short: its bucket index |digit| - 1 stays below 2^tb, a property of the plan and not of the data.
// bound_log2_x1000 > 0 (endomorphism split): every half scalar is at most 2^(bound_log2_x1000 / 1000), so its top
// window holds at most floor(2^e), e = bound - c (W - 1) bits, before the recoding carry of 1 -- an index of at most
// floor(2^e) < 2^(floor(e) + 1).  Else the scalars are below 2^bits: the top window holds at most 2^(bits - c (W - 1)) - 1,
// and with the carry the index stays below that power of two.  A window above the scalar sees the carry alone (index 0).
inline int top_window_bits(int bound_log2_x1000, int bits, int c, int W) {
    int tb;
    if (bound_log2_x1000 > 0) {
        const long e = (long)bound_log2_x1000 - 1000L * c * (W - 1);
        tb = e < 0 ? 0 : (int)(e / 1000) + 1;
    } else {
        tb = bits - c * (W - 1);
    }
    return tb < 0 ? 0 : tb > c - 1 ? c - 1 : tb;
}
// The two-level sort of that window drops delta = min(fb, (c - 1) - tb) of its fine bits: coarse bin = index >> (fb -
// delta), so that the 2^hb bins of the window are cut by the bits it really has and fill evenly, each with 2^(fb - delta)
// fine buckets.  The bucket index itself is unchanged.  AMDMSM_SORT_TOPSHIFT=0: no shift (A/B runs).
inline int sort_top_shift(int tb, int c, int W, int fb) {
    static const bool on = !(getenv("AMDMSM_SORT_TOPSHIFT") && atoi(getenv("AMDMSM_SORT_TOPSHIFT")) == 0);
    if (!on || W < 2) return 0;
    const int spare = c - 1 - tb;
    return spare < fb ? spare : fb;
}

// Queues of buckets whose entries span several accumulation lanes (k_accumulate_fixup):
// spans of more than 32 lanes ("long") and of 3..32 lanes ("mid"), `lanes` = W * T.
#ifdef __HIPCC__
#define AMDMSM_HD __host__ __device__
#else
#define AMDMSM_HD
#endif
AMDMSM_HD inline size_t fixup_queue_cap_long(size_t lanes) { return lanes / 32 + 2; }
AMDMSM_HD inline size_t fixup_queue_cap_mid(size_t lanes) { return lanes / 3 + 2; }
inline size_t fixup_queue_words(size_t lanes) { return 2 + 2 * (fixup_queue_cap_long(lanes) + fixup_queue_cap_mid(lanes)); }

// The buffers of one two-level sort (group_vtable::sort), every pointer the start of window 0 of the call: a sub-range
// of windows, or one MSM of a batch, is sorted by passing offset pointers and its window count.
struct sort_bufs {
    uint32_t* coarse;        // W * SORT_COARSE_WORDS words, zeroed
    uint32_t* cursor;        // W * SORT_CURSOR_WORDS words, zeroed
    int32_t* digits;         // W * stride words; may alias lists (the digits are dead once the coarse pass has run)
    uint32_t* tmp_payload;   // W * stride words
    uint32_t* tmp_key;       // W * stride 16-bit fine keys
    uint32_t* ends;          // out: ends[w][b], W * 2^(c-1) words
    uint32_t* lists;         // out: lists[w][...], W * stride words
    size_t stride;           // words between two windows of digits / tmp_payload / tmp_key / lists
    uint32_t* big;           // sort_geometry().big_words words, the first 4 zeroed (oversized coarse bins, sorted cooperatively)
};
// Where scalar i of a sort comes from.  OWN: record i of `scalars` (Fr records; mont: Montgomery residues).
// SELECTED (amdmsm_*_batch_items): `scalars` is a vector of sel.shared_n scalars that several MSMs share, and base i
// takes element sel.index[i] of it (index != null; any order, repeats allowed), else element sel.offset + i.  An element
// at or past shared_n is not read: it counts as scalar 0 and sets *sel.flag (one word, cleared by the caller) to nonzero.
// SHORT (amdmsm_*_short): W is sized for scalars below 2^shrt.limit_bits, and `scalars` holds elements of shrt.kind =
// AMDMSM_SCALAR_*: 0 = Fr records, else the bytes of one packed little-endian unsigned integer (1, 2, 4, 8; the pointer
// needs that alignment only).  A scalar that is not below the limit counts as 0 and sets *shrt.flag (one word, cleared by
// the caller) to nonzero; limit_bits at the kind's full width tests nothing and the flag may be null.
// The rules: the short form runs mode 0 only; the short form and selection exclude each other (one `form`); and in every
// form sort_bufs::digits may alias sort_bufs::lists.
struct sort_src {
    enum form_t : int { OWN = 0, SELECTED = 1, SHORT = 2 };
    struct selection { const uint32_t* index; size_t offset, shared_n; uint32_t* flag; };   // index null: slice
    struct short_form { int kind, limit_bits; uint32_t* flag; };
    const void* scalars;
    form_t form;
    selection sel;      // SELECTED
    short_form shrt;    // SHORT
    static sort_src own(const uint32_t* scalars) { return {scalars, OWN, {}, {}}; }
    static sort_src selected(const uint32_t* shared, size_t shared_n, const uint32_t* index, size_t offset, uint32_t* flag) {
        return {shared, SELECTED, {index, offset, shared_n, flag}, {}};
    }
    static sort_src short_scalars(const void* scalars, int kind, int limit_bits, uint32_t* flag) {
        return {scalars, SHORT, {}, {kind, limit_bits, flag}};
    }
};

// One pass of amdmsm_group_matrix_apply over the wave jobs job0 .. job0 + n_jobs - 1 of a resident Fr matrix
// (fr_matrix_layout.h; group_matrix.inc).  words, desc, lane_rows: the handle's arrays.  points: at least n_cols compact
// affine records.  prod: the records of the general entries of these jobs, record (rank - first_rank) for the entry of
// rank `rank` in the handle's side array -- gm_gather writes the entry's point there, gm_apply reads its product.
// out: libff records in `form`, one per row; partial: (X, Y, ZZ, ZZZ) records, 4 * el_words words each.
struct gm_args {
    const uint32_t* words;
    const frm_desc* desc;
    const uint32_t* lane_rows;
    const uint32_t* points;
    uint32_t* prod;
    uint32_t* out;
    uint32_t* partial;
    uint32_t job0, n_jobs, first_rank;
    int form;
};

// Members by stage: constants of the group; import / export / codecs; digits and sort; accumulate and fix-up; reduction
// and Horner; fixed-base; point-vector entries (smv, seg, fold, fft, gm); test hooks and probes.  msm_group.hip fills the
// table by member name.
struct group_vtable {
    // ---- constants of the group ----------
    int curve, group;
    int fr_words;      // 32-bit words per scalar
    int el_words;      // 32-bit words per coordinate (Fq or Fq2)
    int fq_words;      // 32-bit limbs of the base prime field
    int fr_bits;       // bit length of the scalar-field modulus
    int projective;    // libff stores this group in homogeneous projective coordinates
    int reduce_fold;   // segments / points one wave of reduce_segments / sum_butterfly folds (64 or 32)
    int bucket_words;  // words between two records of the bucket / partial accumulator arrays (>= 4 * el_words)
    const uint32_t* fr_one_mont;   // Fr::one() in Montgomery form (R mod r), fr_words words
    const uint32_t* fr_modulus;    // the scalar-field modulus r, plain integer, fr_words words
    // the group has the endomorphism phi below (0: MNT4 / MNT6, whose glv_* entries are placeholders and whose
    // amdmsm_opts.endomorphism is ignored); the curve has a != 0 (the compressed-record decoders assume a = 0)
    int has_endomorphism;
    int coeff_a_nonzero;
    // endomorphism split k = k1 + k2 lambda (mod r), phi(x, y) = (beta x, y) = [lambda](x, y) on the
    // order-r subgroup (msm_group.hip glv_split): |k1|, |k2| <= 2^(glv_bound_log2_x1000 / 1000)
    int glv_bound_log2_x1000;
    int prime_order;               // the whole curve group has order r (cofactor 1): phi = [lambda] everywhere
    const uint32_t* glv_lambda;    // plain integer, fr_words words

    // ---- import / export / codecs ----------
    // libff (X, Y, Z) records -> compact affine (x, y); (0, 0) = infinity.
    // form_special != 0 promises Z == 1 or zero (multi_exp_base_form_special).
    void (*import_bases)(hipStream_t, const uint32_t* src, size_t stride_words, int form_special,
                         size_t n, uint32_t* dst_affine);
    // compact affine -> libff special-form records (x, y, 1) / (0, 1, 0)
    void (*export_affine)(hipStream_t, const uint32_t* src_affine, size_t n, uint32_t* dst_xyz);
    // synthetic bases: dst[i] = (first + i + 1) * G::one(), compact affine
    void (*gen_bases_seq)(hipStream_t, unsigned long long first, size_t n, uint32_t* dst_affine);
    // out[i] = phi(P_i) = (beta x_i, y_i), compact affine like the n bases
    void (*endo_points)(hipStream_t, const uint32_t* bases_affine, size_t n, uint32_t* out);
    // table[i*D + j] = [2^(j*c)] P_i (compact affine), j < D; tmp: n*D affine-sized slots of scratch
    void (*precompute_table)(hipStream_t, const uint32_t* bases_affine, size_t n, int c, int D, uint32_t* tmp,
                             uint32_t* table);
    // libff FFI wire format (big-endian plain affine, ffi_serialization.tcc) <-> engine layout;
    // *status receives OR of: 1 out of range, 2 not on curve, 4 not in the safe subgroup
    void (*ffi_decode_points)(hipStream_t, const uint32_t* src_be, size_t n, uint32_t* dst_affine, uint32_t* status);
    void (*ffi_decode_scalars)(hipStream_t, const uint32_t* src_be, size_t n, uint32_t* dst_plain, uint32_t* status);
    void (*ffi_encode_point)(hipStream_t, const uint32_t* src_xyz_affine, uint32_t* dst_be);
    // libff on-disk base records (binary, Montgomery, uncompressed) -> compact affine
    void (*disk_decode)(hipStream_t, const uint32_t* src, size_t n, uint32_t* dst_affine);
    // the compressed form of the same records (X with two flag bits, Y by square root);
    // *status |= 2 where X is not the abscissa of a curve point
    void (*disk_decode_compressed)(hipStream_t, const uint32_t* src, size_t n, uint32_t* dst_affine, uint32_t* status);
    // compact affine -> the same on-disk records, n * 2 * el_words words; the compact zero (0, 0) is written as (0, one)
    void (*disk_encode)(hipStream_t, const uint32_t* src_affine, size_t n, uint32_t* dst);
    // ... and their compressed form, n * el_words words: X with the two flag bits, zero as X = 0 with flag 2 (a = 0 curves)
    void (*disk_encode_compressed)(hipStream_t, const uint32_t* src_affine, size_t n, uint32_t* dst);

    // ---- digits and sort ----------
    // stats[0] += #scalars equal to zero, stats[1] += #scalars equal to one (multi_exp_filter_one_zero's
    // classification, multiexp.tcc:713-733); mont: the scalars are Montgomery residues
    void (*scalar_stats)(hipStream_t, const uint32_t* scalars, size_t n, int mont, uint32_t* stats);
    // Scalars known to be short (amdmsm_*_short), kind as for sort_src's short form (mont as for `sort`).
    // *out_bits = max(*out_bits, bit length of the longest scalar); one word, cleared by the caller
    void (*scalar_bits)(hipStream_t, const void* scalars, int kind, size_t n, int mont, uint32_t* out_bits);
    // out[i] = the scalar base i selects, copied as it is stored (same selection and guard as sort_src's selecting form)
    void (*gather_scalars)(hipStream_t, const uint32_t* shared, size_t shared_n, const uint32_t* index, size_t offset,
                           uint32_t* flag, size_t n, uint32_t* out);
    // histogram of signed radix-2^c digits: counts[w * B + (|d| - 1)]++
    void (*count)(hipStream_t, const uint32_t* scalars, size_t n, int mont, int c, int W, uint32_t* counts);
    // cursor[] holds exclusive bucket starts on entry, bucket ends on exit
    void (*scatter)(hipStream_t, const uint32_t* scalars, size_t n, int mont, int c, int W, uint32_t* cursor,
                    uint32_t* lists, size_t list_stride);
    // LDS-staged two-level sort (same result as count + scatter) of the n scalars of `src` into ends[w][b] and
    // lists[w][...] of `bufs`; needs c <= 22
    // mode 2: endomorphism split -- scalar i yields digit columns i (k1) and n + i (k2), so every
    // per-column array is sized for 2n columns (stride >= 2n) and payloads >= n name phi(P_(e - n))
    // mode 1 (flat): the W digits of scalar i become entries i*W .. i*W+W-1 of ONE list over one
    // bucket set (their payload indexes a precompute_table); then stride >= n*W, coarse / cursor /
    // ends are those of a single window and big is sized by sort_geometry(n*W, c, 1)
    void (*sort)(hipStream_t, const sort_src& src, size_t n, int mont, int c, int W, const sort_bufs& bufs, int mode);
    // The top window of the sort that `sort` runs for (mode, mont, c, W) over `columns` digit columns per window (every
    // form but the short one, whose windows are sized by the data): returns the fine bits dropped there (sort_top_shift)
    // -- the very value the launcher passes to its kernels -- and, in *tb (may be null), the bound on that window's index
    // bits it rests on.  The bound covers every input the entry points admit: the halves of the split obey theirs for any
    // scalar of fr_words words; Montgomery scalars come out of the conversion below r; plain scalars without the split may
    // be any integer of fr_words words (k >= r is documented input), so there only the word length bounds the top window.
    int (*sort_top_window)(int mode, int mont, int c, int W, size_t columns, int* tb);

    // ---- accumulate and fix-up ----------
    // segmented bucket sums: lane t of window w owns list entries [t*S, (t+1)*S); buckets[]
    // must be zero-filled; part_first / part_last: W*T points, cont_bucket: W*T words.
    // Every array argument is the start of window 0 of the call, so a sub-range of windows is
    // processed by passing offset pointers and its window count.
    void (*accumulate)(hipStream_t, const uint32_t* ends, const uint32_t* lists, size_t list_stride,
                       const uint32_t* bases_affine, uint32_t* buckets, uint32_t* part_first, uint32_t* part_last,
                       uint32_t* cont_bucket, int W, uint32_t B, uint32_t S, uint32_t T, const uint32_t* endo_points,
                       size_t n_real, int overlap);
    // overlap != 0 (only where accumulate_overlap_ok): launched one workgroup per CU short of full occupancy, wave
    // priorities one level down, so that a wave of another MSM's tail kernels fits and wins on every SIMD
    // endo_points != null: list entries >= n_real name phi(P_(e - n_real)) = endo_points[e - n_real]
    // lanes of k_accumulate the device holds at once (CUs x resident workgroups x workgroup size)
    size_t (*accumulate_resident_lanes)(int overlap);
    int accumulate_overlap_ok;   // the tail kernels of this group were built to fit beside an overlap-mode accumulation
    // closes the buckets that span several lanes; queue: fixup_queue_words(W*T) words, the
    // first two zeroed
    void (*accumulate_fixup)(hipStream_t, const uint32_t* ends, uint32_t* buckets, uint32_t* part_first,
                             const uint32_t* part_last, const uint32_t* cont_bucket, uint32_t* queue, int W,
                             uint32_t B, uint32_t S, uint32_t T);

    // ---- reduction and Horner ----------
    // M = B/L segments per window, G = min(M, reduce_fold):
    // out[w][g] = sum over segments s in [g*G, (g+1)*G) of sum_j (s*L + j + 1) * bucket[w][s*L + j]
    void (*reduce_segments)(hipStream_t, const uint32_t* buckets, int W, uint32_t B, uint32_t L, uint32_t* out);
    // out[w][g] = sum_{i in [g*G, (g+1)*G)} in[w][i], G = min(M, reduce_fold)
    void (*sum_butterfly)(hipStream_t, const uint32_t* in, int W, uint32_t M, uint32_t* out);
    // out[w] = sum_i in[w][i], i < M, one workgroup per window; M * (64 / reduce_fold) <= 256
    void (*sum_block)(hipStream_t, const uint32_t* in, int W, uint32_t M, uint32_t* out);
    // The bucket reduction as plain sums (msm_group.hip k_bucket_sums / k_plane_sums / k_window_horner):
    // out[w] = sum_b (b + 1) * bucket[w][b].  B = 2^(c-1); q_row / q_col: buckets a lane adds serially in
    // the row / column sums (rounded to what the butterfly width admits); rc: W * (R + 1 + C) points and
    // planes: W * c points of scratch, C = 2^ceil((c-1)/2), R = B / C
    void (*reduce_rowcol)(hipStream_t, const uint32_t* buckets, int W, uint32_t B, int c, uint32_t q_row, uint32_t q_col,
                          uint32_t* rc, uint32_t* planes, uint32_t* out);
    // Horner over window sums (high to low, c doublings between), write one point; init (engine
    // Jacobian, may be null) = value carried in from the windows above window_sums[W-1]
    void (*horner)(hipStream_t, const uint32_t* window_sums, int W, int c, int form, const uint32_t* init,
                   uint32_t* out);
    // the same for k MSMs at once: MSM j's W window sums start at window_sums[j * W], its result goes to outs[j]
    // (k <= 8; one wave per MSM, all chains side by side)
    void (*horner_batch)(hipStream_t, const uint32_t* window_sums, int k, int W, int c, int form, uint32_t* const* outs);
    // sum of k engine-Jacobian points
    void (*sum_points)(hipStream_t, const uint32_t* pts, int k, int form, uint32_t* out);

    // ---- fixed-base ----------
    // fixed-base batch exponentiation: out[i] = (coeff *) scalars[i] * g via a window table
    // (get_window_table / windowed_exp / batch_exp[_with_coeff], multiexp.tcc:809-947);
    // gouter: outerc points, table: outerc * 2^window points (scratch: must be zero-filled), table_aff: as many compact
    // affine records, outerc = ceil(scalar_size / window); build_table = 0 reuses table_aff as a previous call left it
    void (*fixed_base_exp)(hipStream_t, const uint32_t* g_xyz, int scalar_size, int window, const uint32_t* scalars,
                           size_t n, int mont, const uint32_t* coeff, int form, uint32_t* gouter, uint32_t* table,
                           uint32_t* table_aff, int build_table, uint32_t* out);

    // ---- point-vector entries (smv, seg, fold, fft) ----------
    // Element-wise scalar multiplication out[i] = k_i * P_i (amdmsm_scalar_mul_vec), one lane per element.
    // smv_table: table[j * n + i] = (j + 1) * P_i as compact affine records, j < smv_entries ((0, 0) = infinity); tmp: as
    // many records of scratch.  smv_ladder: signed fixed-window ladder over that table; scalars as for `sort` (a plain
    // scalar may be any integer of fr_words words), out: n records in `form` (OUT_AFFINE inverts once per lane: the engine
    // asks for OUT_LIBFF and normalises the batch).
    int smv_entries;
    void (*smv_table)(hipStream_t, const uint32_t* bases_affine, size_t n, uint32_t* tmp, uint32_t* table);
    void (*smv_ladder)(hipStream_t, const uint32_t* table, size_t n, const uint32_t* scalars, int mont, int form, uint32_t* out);

    // Segmented MSM out[j] = sum of k_t * P_t over segment j (amdmsm_multi_exp_segments), over smv_table's records and
    // the ladder's signed 4-bit digits, seg_windows of them per scalar.
    // seg_digits: digits[t * seg_digit_stride + w] = digit w of scalar t, one signed byte each (n * seg_digit_stride bytes).
    // seg_accumulate: one lane per (slice, window).  slices[4 s ..] = (first term, end term, table column of the first
    // term, unused): terms index `digits`, columns the table's rows of nt records; sums: n_slices * seg_windows
    // (X, Y, ZZ, ZZZ) records of 4 * el_words words.
    // seg_fold: winsum[seg * seg_windows + w] = sum over the slices [seg_first[seg], seg_first[seg + 1]) of their window
    // sum w, engine Jacobian (seg_first: m + 1 words).  seg_horner: out[seg] = Horner over the segment's window sums in
    // `form`, one wave per segment (m < 2^31).
    int seg_windows, seg_digit_stride;
    void (*seg_digits)(hipStream_t, const uint32_t* scalars, size_t n, int mont, uint32_t* digits);
    void (*seg_accumulate)(hipStream_t, const uint32_t* table, size_t nt, const uint32_t* digits, const uint32_t* slices,
                           size_t n_slices, uint32_t* sums);
    void (*seg_fold)(hipStream_t, const uint32_t* sums, const uint32_t* seg_first, size_t m, uint32_t* winsum);
    void (*seg_horner)(hipStream_t, const uint32_t* winsum, size_t m, int form, uint32_t* out);

    // Fold of k point vectors by k shared scalars, out[i] = sum_j s_j * P_j[i] (amdmsm_fold_vec), k <= FOLD_MAX_K.
    // fold_digits: the signed 4-bit digits of the k scalars -- HOST memory, k records of fr_words words, passed to the
    // kernel by value -- one signed byte each, digits[row * fold_digit_stride + w], w < W.  glv == 0: row j belongs to
    // P_j and W = seg_windows (the carry digit included: a plain scalar may be any integer of fr_words words);
    // glv != 0: rows 2 j and 2 j + 1 are the halves of the split and belong to P_j and phi(P_j), W windows cover the
    // split's bound.  FOLD_DIGIT_BYTES bytes are enough for every k.  The rows are laid out as seg_digits lays them out,
    // so fold_digit_stride has the value of seg_digit_stride.
    // fold_ladder: one lane per element and one doubling chain for all rows, from the highest window in which some row
    // has a nonzero digit.  tables: the k tables of smv_table one after the other (smv_entries * n records each);
    // rows = k or 2 k; out: n records in `form` as for smv_ladder.
    int fold_digit_stride;
    void (*fold_digits)(hipStream_t, const uint32_t* scalars_host, int k, int mont, int glv, int W, uint32_t* digits);
    void (*fold_ladder)(hipStream_t, const uint32_t* tables, size_t n, const uint32_t* digits, int rows, int glv, int W,
                        int form, uint32_t* out);

    // Radix-2 FFT over a point vector, out[j] = sum_i w^(i j) P_i (amdmsm_group_fft): autosorting decimation-in-time
    // stages, one lane per butterfly.  Butterfly b < n / 2 of the stage with rsh = log2(n) - 1 - stage reads
    // A = in[b + (b >> rsh << rsh)], B = in[that + 2^rsh] (compact affine) and w = twiddles[b >> rsh << rsh], and writes
    // the libff records A + w B to out[b] and A - w B to out[b + half], half = n / 2.
    // fft_gather: dst[i] = B of butterfly b0 + i, i < cn -- the base vector of smv_table.
    // fft_butterfly: butterflies b0 .. b0 + cn - 1; table = smv_table's records of those cn B operands, or null for the
    // stage whose twiddles are all 1 (rsh = log2(n) - 1: T = B, twiddles is not read).  Scalars as for smv_ladder.
    void (*fft_gather)(hipStream_t, const uint32_t* in_affine, size_t b0, size_t cn, int rsh, uint32_t* dst_affine);
    void (*fft_butterfly)(hipStream_t, const uint32_t* table, size_t cn, const uint32_t* in_affine, size_t b0, int rsh,
                          const uint32_t* twiddles, int mont, size_t half, uint32_t* out);

    // Sparse matrix times point vector over the resident form of an Fr matrix (amdmsm_group_matrix_apply), one wave per
    // job.  gm_gather: the points of the jobs' general entries into a.prod, in rank order -- the base vector of
    // smv_table, whose ladder runs with the handle's coefficients.  gm_apply: the row sums of the jobs -- +-points[col]
    // for the entries of coefficient 1 and r - 1, a.prod[rank - first_rank] (compact affine again) for a general one.
    // gm_combine: out[comb[i].row] = the sum of its partials, one lane per split row.
    void (*gm_gather)(hipStream_t, const gm_args& a);
    void (*gm_apply)(hipStream_t, const gm_args& a);
    void (*gm_combine)(hipStream_t, const frm_comb* comb, uint32_t n_comb, const uint32_t* partial, int form, uint32_t* out);

    // ---- test hooks (parity of the primitives against the oracle) ----------
    // coordinate-field op over arrays: 0 mul 1 sqr 2 add 3 sub 4 neg 5 inverse
    void (*field_op)(hipStream_t, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n);
    // group op over arrays of libff-layout records (Jacobian groups: same formulas as
    // libff; bw6_761: converted through affine): 0 add 1 mixed_add 2 dbl; out in `form`
    void (*group_op)(hipStream_t, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, int form);
    // signed digits of each scalar: out[i * W + w]
    void (*digits)(hipStream_t, const uint32_t* scalars, size_t n, int mont, int c, int W, int32_t* out);
    // signed digits of both halves of the endomorphism split, out[(2 i + half) * W + w]
    void (*glv_digits)(hipStream_t, const uint32_t* scalars, size_t n, int mont, int c, int W, int32_t* out);
    // throughput probes: 2*iters dependent Fq products / iters mixed additions per lane
    // (inline_variant selects the fully inlined product where the TU was built with it)
    void (*mul_bench)(hipStream_t, uint32_t* inout, size_t nthreads, int iters, int inline_variant);
    void (*madd_bench)(hipStream_t, const uint32_t* pts_affine, uint32_t* out_xyz, size_t nthreads, int iters,
                       int inline_variant);

    // ---- probes of the field and point layers (tests/test_gpu_field_probe.py) ----------
    // One library function (FPROBE_*) per element on the cold element type (impl 0) or the fully inlined one (impl 1):
    // operands a, b, c, d (null where the op takes fewer) and out are n elements of el_words words, taken and stored as
    // they are; flag (may be null): one word per element, the boolean the op returns (else 0).
    void (*field_probe)(hipStream_t, int impl, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                        const uint32_t* d, uint32_t* out, uint32_t* flag, size_t n);
    // One extended-Jacobian function (XPROBE_*) per lane: acc and out are n (X, Y, ZZ, ZZZ) records of 4 * el_words
    // words; pt: n compact affine records, or n more (X, Y, ZZ, ZZZ) records for XPROBE_ADD (null where unused)
    void (*xyzz_probe)(hipStream_t, int impl, int op, const uint32_t* acc, const uint32_t* pt, uint32_t* out, size_t n);
    // ---- probes of the reduced-radix layer, rr.cuh (tests/test_gpu_rr_probe.py); null where the group does not
    // accumulate on it (the MNT units) ----------
    // One function (RRPROBE_*) per element on RAW limbs.  Rows: one per Fq component, n rows for an Fq group, 2 n for an
    // Fq2 group (element i = rows 2 i, 2 i + 1 = c0, c1, served by a lane pair).  a, b, c, d: rows of L limbs (null:
    // zeros); w: rows of fq_words words (null: zeros); out: rows of L limbs; outw: rows of fq_words words; flag: one word
    // per ELEMENT; k: the factor of RRPROBE_SMALL_TIMES.
    void (*rr_probe)(hipStream_t, int op, int k, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                     const uint32_t* w, int32_t* out, uint32_t* outw, uint32_t* flag, size_t n);
    // One step of one point function (XRRPROBE_*) per element.  acc, sec (null: zeros), out: rows of 4 L limbs (x, y, zz,
    // zzz; the Jacobian ops: x, y, z, 0); pt (null: zeros): rows of 2 fq_words words (affine x, y); fin (null: zeros), fout:
    // one word per element -- fin bit 0: acc is infinity, bit 1: sec is, bit 2: subtract; fout bit 0: the result is
    // infinity, bit 1: jac_is_inf_rr; outw: rows of 4 fq_words words, the result exported (zeros for infinity).
    void (*xyzz_rr_probe)(hipStream_t, int op, const int32_t* acc, const int32_t* sec, const uint32_t* pt, const uint32_t* fin,
                          int32_t* out, uint32_t* outw, uint32_t* fout, size_t n);
    int rr_probe_first_reduced;   // the unit carries RRPROBE_FIRST_REDUCED (the table of multiples of p is built: D <= 8)
};
constexpr int FOLD_MAX_K = 8;
constexpr size_t FOLD_DIGIT_BYTES = 2048;   // 2 FOLD_MAX_K rows of at most 100 bytes

// op codes of field_probe: canonical operands in [0, p) per component ...
enum {
    FPROBE_MUL = 0, FPROBE_SQR = 1, FPROBE_ADD = 2, FPROBE_SUB = 3, FPROBE_NEG = 4, FPROBE_INV = 5, FPROBE_DBL = 6,
    FPROBE_CNEG = 7,       // negates where the low bit of b's first word is set
    FPROBE_HALF = 8, FPROBE_TO_MONT = 9, FPROBE_FROM_MONT = 10,
    FPROBE_SQRT = 11,      // flag: a is a square (out: either root)
    // ... and the almost-reduced set: operands in [0, 2p) per component, results below 2p
    FPROBE_MUL_LZ = 16, FPROBE_SQR_LZ = 17, FPROBE_SUB_LZ = 18, FPROBE_ADD_LZ = 19, FPROBE_NEG_LZ = 20,
    FPROBE_MUL_SUB_MUL_LZ = 21,   // a b - c d
    FPROBE_IS_ZERO_LZ = 22,       // flag
    FPROBE_CANON = 23,
};
enum { XPROBE_MADD_LZ = 0, XPROBE_MADD = 1, XPROBE_ADD = 2, XPROBE_DBL = 3, XPROBE_DBL_AFFINE = 4, XPROBE_TO_JAC = 5 };
// op codes of rr_probe (include/amdmsm.h amdmsm_rr_probe_device): the products ...
enum {
    RRPROBE_MUL = 0,             // rr_mul(a, b), per component
    RRPROBE_MUL2 = 1,            // rr_mul2: a b + c d
    RRPROBE_SQR = 2,             // rr_sqr(a)
    RRPROBE_RE_MUL = 3,          // re_mul on the element (Fq2: over the lane pair)
    RRPROBE_RE_SQR = 4,
    RRPROBE_RE_MUL_SUB_MUL = 5,  // a b - c d
    RRPROBE_MUL_POW2_32N = 6,    // rr_mul_pow2<32 N>
    RRPROBE_MUL_POW2_32N_D = 7,  // rr_mul_pow2<32 N - D>
    RRPROBE_FROM_WORDS_RHO = 8,  // re_from_words_rho(w)
    RRPROBE_EXPORT_0 = 9,        // rr_export_component<0>(a) -> outw
    RRPROBE_EXPORT_D = 10,       // rr_export_component<D>(a) -> outw
    // ... and everything else
    RRPROBE_NORM = 16, RRPROBE_RIPPLE = 17,
    RRPROBE_SMALL_TIMES = 18,    // re_small_times(a, k), k = 2, 3, 4
    RRPROBE_CNEG = 19,           // rr_cneg(a, odd element index)
    RRPROBE_FROM_WORDS_0 = 20, RRPROBE_FROM_WORDS_D = 21,   // rr_from_words<0 / D>(w)
    RRPROBE_FIRST_REDUCED = 22,  // rr_first_reduced(w)
    RRPROBE_FIRST_COORD = 23,    // re_first_coord(w)
    RRPROBE_TO_WORDS = 24,       // rr_to_words(a) -> outw
    RRPROBE_CANON_PRODUCT = 25,
    RRPROBE_IS_ZERO_EXACT = 26,  // flag: re_is_zero_exact(a)
    RRPROBE_MAYBE_ZERO_K = 27,   // flag: re_maybe_zero<rr_filter_k>(a)
    RRPROBE_MAYBE_ZERO_64 = 28,  // flag: re_maybe_zero<64>(a)
    RRPROBE_SET_POW2_BL = 29, RRPROBE_SET_POW2_BL_D = 30,   // re_set_pow2<B L>, <B L + D>
};
enum {
    XRRPROBE_MADD = 0,           // xyzz_madd_rr(acc, inf, pt, neg)
    XRRPROBE_FIRST = 1,          // xyzz_rr_first(pt, neg)
    XRRPROBE_REC_TO_RHO = 2,     // xyzz_rec_to_rho(acc)
    XRRPROBE_EXPORT = 3,         // acc as it is; outw: the export of a record of k_accumulate (zz, zzz with rho 2^D)
    XRRPROBE_EXPORT_RHO = 4,     // ... of a sum (every coordinate with rho)
    XRRPROBE_DBL_RHO = 8,        // xyzz_dbl_rho(acc, inf)
    XRRPROBE_ADD_RHO = 9,        // xyzz_add_rho(acc, inf, sec, sec_inf)
    XRRPROBE_JAC_DBL = 16,       // jac_dbl_rr(acc, inf)
    XRRPROBE_JAC_MADD = 17,      // jac_madd_rr(acc, inf, sec.x, sec.y)
    XRRPROBE_JAC_IS_INF = 18,    // fout bit 1: jac_is_inf_rr(acc, inf)
};

const group_vtable* vt_alt_bn128_g1() __attribute__((weak));
const group_vtable* vt_alt_bn128_g2() __attribute__((weak));
const group_vtable* vt_bls12_377_g1() __attribute__((weak));
const group_vtable* vt_bls12_377_g2() __attribute__((weak));
const group_vtable* vt_bw6_761_g1() __attribute__((weak));
const group_vtable* vt_bw6_761_g2() __attribute__((weak));
const group_vtable* vt_bls12_381_g1() __attribute__((weak));
const group_vtable* vt_bls12_381_g2() __attribute__((weak));
const group_vtable* vt_mnt4_g1() __attribute__((weak));
const group_vtable* vt_mnt4_g2() __attribute__((weak));
const group_vtable* vt_mnt6_g1() __attribute__((weak));

}  // namespace amdmsm
