// Host-visible interface of one scalar-field translation unit (fr_ntt.hip, compiled once per curve with
// -DAMDMSM_FR=<curve>_fr): the field's constants for the host-side parameter arithmetic of engine.cpp and launchers of
// the kernels.  Every record that crosses this interface on the host side is a Montgomery residue below r.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fr_matrix_layout.h"
#include "fr_scan_layout.h"

namespace amdmsm {

constexpr int FR_MAX_WORDS = 12;
constexpr int FR_LDS_LOG2 = 10;        // records of one LDS tile (log2), every field: 32 / 40 / 48 KiB
constexpr int FR_TILE_MIN = 4, FR_TILE_MAX = 8, FR_TILE_DEFAULT = 8;   // butterfly stages per global pass
constexpr int FR_POW_TABLE = 17;       // base^(2^b), b = 0 .. 16: what k_fr_powers is given
constexpr int FR_LINCOMB_MAX = 4;      // vectors of one linear combination (k_fr_lincomb)

// one global pass of the transform (k_fr_fft_pass): log_r in-LDS stages on tiles of 2^log_c neighbouring columns
struct fr_pass {
    const uint32_t* in;
    uint32_t* out;
    const uint32_t* tw;         // n / 2 powers of omega, Montgomery
    const uint32_t* pre_col;    // first pass, pre given: pre^c, c < n >> log_r;  else null
    const uint32_t* pre_row;    //                        pre^((n >> log_r) k), k < 2^log_r
    const uint32_t* post_col;   // last pass, post given: post^q, q < 2^log_s;  else null
    const uint32_t* post_row;   //                        scale * post^(k << log_s), k < 2^log_r
    int log_n, log_r, log_s, log_c;
    int in_plain, out_plain;    // conversion at the first load / the last store
    int has_scale;              // last pass, scale given and post not: every result times scale
    uint32_t scale[FR_MAX_WORDS];
};

// the same pass over `batch` vectors of one size (k_fr_fft_pass_batch): vector v starts at record v * in_stride of
// p.in and v * out_stride of p.out; the twiddles and the pre / post tables serve every vector.  A workgroup's tile is
// always 2^FR_LDS_LOG2 records: from n = 2^FR_LDS_LOG2 on it is one of the 2^log_tiles tiles of one vector (log_v = 0),
// below that the whole of 2^log_v = 2^FR_LDS_LOG2 / n vectors (log_tiles = 0), the vector index in the tile's upper bits
struct fr_pass_batch {
    fr_pass p;
    size_t in_stride, out_stride;   // records
    uint32_t batch;
    int log_v, log_tiles;
};

// terms added to single records of a vector (k_fr_add_terms): h[idx[k]] += c[k], k < count; with `set`, term 0 is
// stored instead -- the record behind a vector that nothing has written yet.  The indices differ from one another
constexpr int FR_TERMS_MAX = 4;
struct fr_terms {
    size_t idx[FR_TERMS_MAX];
    uint32_t c[FR_TERMS_MAX][FR_MAX_WORDS];   // in the form of the vector's records
    int count, set;
};

// one apply of a resident sparse matrix (k_frm_apply, k_frm_combine; fr_matrix_layout.h has the arrays' meaning)
struct frm_args {
    const uint32_t* words;
    const uint32_t* coef;        // the general coefficients in word order, Montgomery
    const frm_desc* desc;
    const uint32_t* lane_rows;
    const frm_comb* comb;
    const uint32_t* x;
    uint32_t* out;
    uint32_t* partial;           // n_partials records of workspace
    uint32_t n_desc, n_comb;
    size_t n_rows, n_out;        // out[n_rows .. n_out - 1] = 0
};

// one scan or batch inversion (k_frs_reduce, k_frs_spine, k_frs_apply and their inversion forms; fr_scan_layout.h has the
// tiles and the workspace).  Positions, not records: position p is record frs_record(n, reverse, p)
struct frs_args {
    const uint32_t* a;           // has_a == 1: the vector; an inversion: the values
    const uint32_t* b;
    uint32_t* out;
    uint32_t* total;             // one record or null
    uint64_t* zero_count;        // an inversion: the number of zero records, or null
    uint32_t *ws_a, *ws_b, *ws_in, *ws_cnt;   // workspace; the naive inversion: ws_a holds n running products
    size_t n;
    uint32_t tiles;
    int tile_log2;
    int has_a, has_b;            // has_a: 0 = every a_i is 1, 1 = a vector, 2 = a_const
    int reverse, exclusive, plain, invert;
    uint32_t a_const[FR_MAX_WORDS], init[FR_MAX_WORDS];   // Montgomery
};

// one sweep over the K x S matrix of a step-domain transform, m = B + S, K = B / S (k_frd_sweep, fr_domain.inc): a
// workgroup takes 2^log_w columns and (256 >> log_w) * iters rows and leaves one row of partial sums
constexpr int FRD_FOLD = 0, FRD_MERGE = 1, FRD_REDUCE = 2;
constexpr int FRD_LO_LOG2 = 10;        // g^i = g_lo[i mod 2^10] * g_hi[i >> 10]
constexpr int FRD_TILE_LOG2 = 8;       // columns of a workgroup at the most (log2): one lane each
// Rows a lane walks.  A tile is 256 * iters records and leaves 2^log_w sums, partial sums that are written and read
// once more: 1 / ((256 >> log_w) * iters) of the records -- a sixteenth where a lane has a column to itself, a
// thousandth where the 256 lanes share one -- and the shorter walk gives the many-row tiles four times the workgroups
constexpr uint32_t FRD_ITERS_REDUCE = 64;
inline uint32_t frd_iters(int log_w) { return log_w >= 7 ? 16 : (log_w >= 5 ? 8 : 4); }
struct frd_sweep {
    const uint32_t* in;          // fold: the m input records; merge: U0 | U1, the output vector; reduce: rows x S partial sums
    uint32_t* out;               // fold: c_i to out[i]; merge: a_i to out[i], rows 1 .. K - 1 (may be in)
    uint32_t* sums;              // ceil(rows / ((256 >> log_w) * iters)) rows of S sums
    const uint32_t* tw;          // the B powers of w, Montgomery (fold, merge)
    const uint32_t *g_lo, *g_hi; // a coset: the powers of g (fold) or of 1 / g (merge), else null
    int log_b, log_s, log_w, mode;
    uint32_t rows, iters;
    int plain;                   // fold: the input is plain; merge: the output is
    int store;                   // rows 1 .. K - 1 are written: the records change or go to another vector
};
// row 0 of the inverse (k_frd_combine): out[i], out[B + i], i < S, from U0_i, U1_i and the sums
struct frd_combine {
    uint32_t* out;
    const uint32_t *sums, *tw, *g_lo, *g_hi;
    int log_b, log_s, plain;
    uint32_t half[FR_MAX_WORDS];   // 1 / 2, Montgomery
};
// the Lagrange vector of a domain at a point t (k_frd_lagrange): m denominators 1 / L_j(t) for the batch inversion, or
// with `unit` (Z(t) = 0) the unit vector itself.  A basic domain has step = 0, log_o = log2 m and no K-table
struct frd_lagrange {
    const uint32_t* tw;          // the 2^(log_o - 1) powers of the root of order 2^log_o, Montgomery
    const uint32_t* kden;        // step: the K factors of the records below B
    uint32_t* out;               // m records
    size_t m;
    int log_b, log_s, log_o, step, unit;
    uint32_t t[FR_MAX_WORDS];    // Montgomery
    uint32_t tail[FR_MAX_WORDS]; // the factor from B on (basic: of every record); unit: what a 1 is in the caller's form
};

// Members by stage: constants of the field, the transform, the sparse matrix, scans, step domains.  fr_ntt.hip fills
// the table by member name.
struct fr_vtable {
    int curve, words, two_adicity;
    uint32_t inv;                                  // -r^-1 mod 2^32
    const uint32_t *modulus, *one, *r2, *root;     // r, R mod r, R^2 mod r, libff's Fr::root_of_unity (Montgomery)
    const uint32_t* generator;                     // libff's Fr::multiplicative_generator (Montgomery): the step domains' coset
    // d_out[i] = first * base^i, i < n.  table: FR_POW_TABLE host records base^(2^b); first: a host record or null (1)
    void (*powers)(hipStream_t, const uint32_t* table, const uint32_t* first, int out_plain, size_t n, uint32_t* d_out);
    void (*pass)(hipStream_t, const fr_pass&);
    // d_out[i] = (a_i * b_i - c_i) * k; d_c, k: null for 0 and 1.  k: a host record
    void (*muladd)(hipStream_t, size_t n, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, const uint32_t* k,
                   int plain, uint32_t* d_out);
    // d_out[i] = sum over j < k of s_j * v_j[i], 1 <= k <= FR_LINCOMB_MAX.  d_v: k device vectors in host memory, any of
    // them d_out; scalars: k packed host records.  Records keep the form they come in
    void (*lincomb)(hipStream_t, size_t n, int k, const uint32_t* const* d_v, const uint32_t* scalars, uint32_t* d_out);
    // sparse matrix times vector: general products summed unreduced, matrix_chunk of them to one Montgomery reduction
    uint32_t matrix_chunk;
    void (*matrix_apply)(hipStream_t, const frm_args&);
    // the same from the caller's CSR (coefficients Montgomery), one lane per row: AMDMSM_FR_MATRIX_NAIVE=1
    void (*matrix_naive)(hipStream_t, size_t n_rows, size_t n_out, const uint64_t* d_offsets, const uint32_t* d_cols,
                         const uint32_t* d_coef, const uint32_t* d_x, uint32_t* d_out);
    // y_i = a_i y_(i-1) + b_i over the positions, or out[i] = 1 / a[i]: reduce, spine, apply in stream order
    void (*scan)(hipStream_t, const frs_args&);
    // the same by one lane that walks the vector: AMDMSM_FR_SCAN_NAIVE=1
    void (*scan_naive)(hipStream_t, const frs_args&);
    // step radix-2 domains (fr_domain.inc): the fold / merge / partial-sum sweep, row 0 of the inverse, d_den[k] -= c
    // (c: a host record), and d_out[j] = d_in[j] * (j < B ? d_inv[j mod K] : tail) for j < m (tail: a host record;
    // B = 0: tail throughout)
    void (*domain_sweep)(hipStream_t, const frd_sweep&);
    void (*domain_combine)(hipStream_t, const frd_combine&);
    void (*domain_den)(hipStream_t, size_t n, uint32_t* d_den, const uint32_t* c);
    void (*domain_divide)(hipStream_t, size_t m, size_t B, size_t K, const uint32_t* d_in, const uint32_t* d_inv, const uint32_t* tail,
                          uint32_t* d_out);
    // record j of the domain's Lagrange vector at t, as its denominator or, on a point of the domain, as it is
    void (*domain_lagrange)(hipStream_t, const frd_lagrange&);
    // one pass over a batch of vectors of one size; batch >= 1
    void (*pass_batch)(hipStream_t, const fr_pass_batch&);
    // d_h[idx[k]] += c[k] (term 0 stored with `set`): the Z terms behind a quotient
    void (*add_terms)(hipStream_t, const fr_terms&, uint32_t* d_h);
};

const fr_vtable* frvt_alt_bn128() __attribute__((weak));
const fr_vtable* frvt_bls12_377() __attribute__((weak));
const fr_vtable* frvt_bw6_761() __attribute__((weak));
const fr_vtable* frvt_bls12_381() __attribute__((weak));
const fr_vtable* frvt_mnt4() __attribute__((weak));
const fr_vtable* frvt_mnt6() __attribute__((weak));

}  // namespace amdmsm
