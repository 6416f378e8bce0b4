// Scalar-field translation unit: the radix-2 FFT over a vector of Fr records, the powers of an Fr element, the
// element-wise product step between transforms, the sparse matrix times vector (fr_matrix.inc), the scans and batch
// inversion (fr_scan.inc) and the sweeps of the step radix-2 domains (fr_domain.inc).  Compiled once per curve:
//   -DAMDMSM_FR=<curve>_fr -DAMDMSM_FR_VT=frvt_<curve> -DAMDMSM_FR_CURVE=<curve id>
// (libff_amd/build.py).  The host side -- plan, argument rules, parameter arithmetic, twiddle cache -- is engine.cpp;
// DESIGN section 18 has the pass structure, the LDS layout and the measurements.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve_params.h"
#include "fp.cuh"
#include "fr_vtable.h"

#if !defined(AMDMSM_FR) || !defined(AMDMSM_FR_VT) || !defined(AMDMSM_FR_CURVE)
#error "compile with -DAMDMSM_FR=<curve>_fr -DAMDMSM_FR_VT=frvt_<curve> -DAMDMSM_FR_CURVE=<curve id>"
#endif

namespace amdmsm {
namespace {

using FR = AMDMSM_FR;
using F = Fp<FR, true>;   // products inlined: the butterfly loop is nothing else
constexpr int N = FR::N;
constexpr int TPB = 256;
constexpr uint32_t E = 1u << FR_LDS_LOG2;
static_assert(N % 2 == 0 && N <= FR_MAX_WORDS, "Fr records are pairs of words, twelve words at the most");
static_assert(FR_TILE_MAX + 2 <= FR_LDS_LOG2, "a strided pass moves at least four neighbouring records per row");

// ---- the LDS tile ---------------------------------------------------------------------------------------------------
// 2^10 records, limb-pair major: word pair w of record L is the uint2 at tile[w][sw(L)], so the lanes of a wave that
// work on consecutive records read and write consecutive 8-byte slots (ds_read_b64 / ds_write_b64).  A read is served
// in groups of 32 lanes that must differ in the slot's low five bits, a write in groups of 16 lanes that must differ in
// its low four.  A butterfly stage whose partner distance 2^a is below 32 records has such a group take the records of
// a span whose bit a is clear; the store phase of a pass reads records that differ in their highest index bits.  sw()
// is a linear map of the index bits onto the slot's low five -- bit 4 also flips bits 2 and 3, bit 5 flips bit 4, bits
// 6, 7, 8 flip bits 1, 2, 3, bit 9 flips bits 4 and 0 -- under which every one of those groups, and every run of
// consecutive records, is conflict-free (tools/fr_fft_lds_conflicts.py counts them, shape by shape).
AMDMSM_DEV uint32_t sw(uint32_t L) {
    const uint32_t x = L >> 5;
    return L ^ (x & 14u) ^ ((x & 1u) << 4) ^ ((x >> 4) * 17u) ^ (((L >> 4) & 1u) * 12u);
}
AMDMSM_DEV void tile_put(uint2 (*tile)[E], uint32_t L, const F& a) {
    const uint32_t s = sw(L);
#pragma unroll
    for (int w = 0; w < N / 2; ++w) tile[w][s] = make_uint2(a.v[2 * w], a.v[2 * w + 1]);
}
AMDMSM_DEV void tile_get(F& r, const uint2 (*tile)[E], uint32_t L) {
    const uint32_t s = sw(L);
#pragma unroll
    for (int w = 0; w < N / 2; ++w) {
        const uint2 v = tile[w][s];
        r.v[2 * w] = v.x;
        r.v[2 * w + 1] = v.y;
    }
}
AMDMSM_DEV void rec_load(F& r, const uint32_t* base, size_t i) { fp_load(r, base + i * (size_t)N); }
AMDMSM_DEV void rec_store(uint32_t* base, size_t i, const F& a) { fp_store(base + i * (size_t)N, a); }
AMDMSM_DEV void rec_copy(F& r, const uint32_t* words) {
#pragma unroll
    for (int w = 0; w < N; ++w) r.v[w] = words[w];
}

// ---- one global pass ------------------------------------------------------------------------------------------------
// The vector is n = 2^log_n records; the passes before this one have done log_s stages (s = 2^log_s), this one does
// t = log_r.  It is one step of the self-sorting (Stockham) radix-2^t transform: with R = 2^t, m = n / (s R), a column
// c = q + s p (q < s, p < m) reads in[c + (n / R) k] and writes out[q + s (R p + k')], k, k' < R, where
//     out_k' = sum_k in_k w^(s k' (p + m k)).
// A workgroup holds the 2^log_c neighbouring columns c0 .. c0 + C - 1 in LDS as record k C + cc, runs the t stages
// there in place, decimation in frequency -- stage j pairs rows k, k + h (h = R >> (j + 1), i = k mod h) with the
// twiddle w^(s 2^j (p + m i)), an index below n / 2 -- and finds row k' at the bit-reversed row of the tile when it
// stores.  Every record is read once and written once; a row of the load is C contiguous records, a row of the store
// min(s, C) R or C of them.
__global__ void __launch_bounds__(TPB) k_fr_fft_pass(const fr_pass a) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    const int ln = a.log_n, t = a.log_r, ls = a.log_s, lc = a.log_c;
    const int lm = ln - ls - t;
    const uint32_t C = 1u << lc, R = 1u << t, Et = 1u << (t + lc);
    const uint32_t c0 = blockIdx.x << lc;

    for (uint32_t e = tid; e < Et; e += TPB) {
        const uint32_t k = e >> lc, c = c0 + (e & (C - 1));
        F v;
        rec_load(v, a.in, (size_t)c + ((size_t)k << (ln - t)));
        if (a.in_plain) fp_to_mont(v, v);
        if (a.pre_col) {
            F f;
            rec_load(f, a.pre_row, k);
            fp_mul(v, v, f);
            rec_load(f, a.pre_col, c);
            fp_mul(v, v, f);
        }
        tile_put(tile, e, v);
    }
    __syncthreads();

    for (int j = 0; j < t; ++j) {
        const int lh = t - 1 - j;
        const uint32_t h = 1u << lh;
        for (uint32_t bf = tid; bf < Et / 2; bf += TPB) {
            const uint32_t cc = bf & (C - 1), x = bf >> lc, i = x & (h - 1), blk = x >> lh;
            const uint32_t lo = ((((blk << (lh + 1)) + i) << lc) | cc), hi = lo + (h << lc);
            const uint32_t p = (c0 + cc) >> ls;
            const size_t tw = ((size_t)p + ((size_t)i << lm)) << (ls + j);
            F u, v, w, d;
            rec_load(w, a.tw, tw);
            tile_get(u, tile, lo);
            tile_get(v, tile, hi);
            fp_sub(d, u, v);
            fp_add(u, u, v);
            fp_mul(d, d, w);
            tile_put(tile, lo, u);
            tile_put(tile, hi, d);
        }
        __syncthreads();
    }

    const int lsp = ls < lc ? ls : lc;
    F scale;
    rec_copy(scale, a.scale);
    for (uint32_t e = tid; e < Et; e += TPB) {
        const uint32_t ql = e & ((1u << lsp) - 1), k2 = (e >> lsp) & (R - 1), pl = e >> (lsp + t);
        const uint32_t cc = (pl << lsp) + ql, c = c0 + cc;
        const uint32_t q = c & ((1u << ls) - 1), p = c >> ls;
        const uint32_t k = t ? __brev(k2) >> (32 - t) : 0u;
        F v;
        tile_get(v, tile, (k << lc) | cc);
        if (a.post_col) {   // last pass: p = 0, the output index is q + s k2
            F f;
            rec_load(f, a.post_row, k2);
            fp_mul(v, v, f);
            rec_load(f, a.post_col, q);
            fp_mul(v, v, f);
        } else if (a.has_scale) {
            fp_mul(v, v, scale);
        }
        if (a.out_plain) fp_from_mont(v, v);
        rec_store(a.out, (size_t)q + ((((size_t)p << t) + k2) << ls), v);
    }
}

// ---- powers of an element -------------------------------------------------------------------------------------------
// out[i] = first * base^i.  The grid has P = 2^log_p lanes; lane g builds first * base^g from the set bits of g and
// the host's table base^(2^b) -- at most log_p + 1 products before its first store -- and then steps by base^P, a
// table entry too, so that a wave's stores stay contiguous.
struct fr_pow_args {
    uint32_t table[FR_POW_TABLE][N];
    uint32_t first[N];
};
__global__ void __launch_bounds__(TPB) k_fr_powers(const fr_pow_args a, int log_p, int out_plain, size_t n,
                                                   uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    F acc, f;
    rec_copy(acc, a.first);
#pragma unroll 1
    for (int b = 0; b < log_p; ++b) {
        rec_copy(f, a.table[b]);
        if ((g >> b) & 1u) fp_mul(acc, acc, f);
    }
    rec_copy(f, a.table[log_p]);
    for (size_t i = g; i < n; i += (size_t)1 << log_p) {
        F v = acc;
        if (out_plain) fp_from_mont(v, v);
        rec_store(out, i, v);
        fp_mul(acc, acc, f);
    }
}

// ---- out[i] = (a_i b_i - c_i) k ---------------------------------------------------------------------------------------
// Plain records: the Montgomery product of two plain integers is a b / R, one more product by R^2 brings a b back; the
// host hands k over as a Montgomery residue either way, which keeps a plain (a b - c) plain.
struct fr_rec_arg {
    uint32_t v[N];
};
__global__ void __launch_bounds__(TPB) k_fr_muladd(size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                   const fr_rec_arg k, int has_k, int plain, uint32_t* out) {
    F kk;
    rec_copy(kk, k.v);
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        F x, y;
        rec_load(x, a, i);
        rec_load(y, b, i);
        fp_mul(x, x, y);
        if (plain) fp_to_mont(x, x);
        if (c) {
            rec_load(y, c, i);
            fp_sub(x, x, y);
        }
        if (has_k) fp_mul(x, x, kk);
        rec_store(out, i, x);
    }
}

// ---- out[i] = sum over j < k of s_j v_j[i] -------------------------------------------------------------------------------
// The scalars are Montgomery residues whatever the vectors are: the Montgomery product of s R and a plain v is the
// plain s v, of s R and v R it is s v R.  A lane reads its record of every vector before it writes, so out may be any
// one of them.
struct fr_lincomb_args {
    const uint32_t* v[FR_LINCOMB_MAX];
    uint32_t s[FR_LINCOMB_MAX][N];
};
__global__ void __launch_bounds__(TPB) k_fr_lincomb(size_t n, int k, const fr_lincomb_args a, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    F acc;
    fp_set_zero(acc);
#pragma unroll
    for (int j = 0; j < FR_LINCOMB_MAX; ++j) {
        if (j < k) {
            F x, s;
            rec_copy(s, a.s[j]);
            rec_load(x, a.v[j], i);
            fp_mul(x, x, s);
            fp_add(acc, acc, x);
        }
    }
    rec_store(out, i, acc);
}

// ---- sparse matrix times vector ---------------------------------------------------------------------------------------
#include "fr_matrix.inc"

// ---- scans and batch inversion ----------------------------------------------------------------------------------------
#include "fr_scan.inc"

// ---- step radix-2 domains: the fold in front of the passes, the merge behind them, the division by Z ----------------
#include "fr_domain.inc"

// ---- one global pass over a batch of vectors ------------------------------------------------------------------------
// k_fr_fft_pass for `batch` vectors of n records that share twiddles and tables; its own copy of the body, so that the
// single-vector kernel stays as the compiler had it (as k_sort_digits_sel).  The LDS tile always holds
// 2^10 records, 2^le of them (le = log_r + log_c) of one vector:
//   n >= 2^10   le = 10.  Workgroup g serves tile g mod 2^log_tiles of vector g >> log_tiles.
//   n <  2^10   le = log_n, c0 = 0.  Workgroup g holds the V = 2^log_v = 2^10 / n vectors g V .. g V + V - 1, vector vl of
//               them in the records vl 2^le .. of the tile; the last workgroup may hold fewer.
// Record e of the tile belongs to vector v0 + (e >> le) and is record e mod 2^le of that vector's tile in k_fr_fft_pass;
// the stage loop and the store order are that kernel's on the low le bits.  A butterfly pairs two records of one vector,
// so the lanes of a vector >= batch skip loads, butterflies and stores alike and still reach every barrier.  Every
// index comes from log_n, the strides, batch and blockIdx: a lane touches records [v stride, v stride + n) of a vector
// v < batch, and twiddle indices stay below n / 2 as in k_fr_fft_pass.
__global__ void __launch_bounds__(TPB) k_fr_fft_pass_batch(const fr_pass_batch b) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    const int ln = b.p.log_n, t = b.p.log_r, ls = b.p.log_s, lc = b.p.log_c;
    const int lm = ln - ls - t, le = t + lc;
    const uint32_t C = 1u << lc, R = 1u << t, Em = (1u << le) - 1;
    const uint32_t c0 = (blockIdx.x & ((1u << b.log_tiles) - 1)) << lc;
    const uint32_t v0 = (blockIdx.x >> b.log_tiles) << b.log_v;

    for (uint32_t e = tid; e < E; e += TPB) {
        const uint32_t vec = v0 + (e >> le), ee = e & Em;
        if (vec >= b.batch) continue;
        const uint32_t k = ee >> lc, c = c0 + (ee & (C - 1));
        F v;
        rec_load(v, b.p.in, (size_t)vec * b.in_stride + c + ((size_t)k << (ln - t)));
        if (b.p.in_plain) fp_to_mont(v, v);
        if (b.p.pre_col) {
            F f;
            rec_load(f, b.p.pre_row, k);
            fp_mul(v, v, f);
            rec_load(f, b.p.pre_col, c);
            fp_mul(v, v, f);
        }
        tile_put(tile, e, v);
    }
    __syncthreads();

    for (int j = 0; j < t; ++j) {
        const int lh = t - 1 - j;
        const uint32_t h = 1u << lh;
        for (uint32_t bf = tid; bf < E / 2; bf += TPB) {
            const uint32_t vl = bf >> (le - 1), bb = bf & (Em >> 1);
            if (v0 + vl < b.batch) {
                const uint32_t cc = bb & (C - 1), x = bb >> lc, i = x & (h - 1), blk = x >> lh;
                const uint32_t lo = (vl << le) | ((((blk << (lh + 1)) + i) << lc) | cc), hi = lo + (h << lc);
                const uint32_t p = (c0 + cc) >> ls;
                const size_t tw = ((size_t)p + ((size_t)i << lm)) << (ls + j);
                F u, v, w, d;
                rec_load(w, b.p.tw, tw);
                tile_get(u, tile, lo);
                tile_get(v, tile, hi);
                fp_sub(d, u, v);
                fp_add(u, u, v);
                fp_mul(d, d, w);
                tile_put(tile, lo, u);
                tile_put(tile, hi, d);
            }
        }
        __syncthreads();
    }

    const int lsp = ls < lc ? ls : lc;
    F scale;
    rec_copy(scale, b.p.scale);
    for (uint32_t e = tid; e < E; e += TPB) {
        const uint32_t vl = e >> le, vec = v0 + vl, ee = e & Em;
        if (vec >= b.batch) continue;
        const uint32_t ql = ee & ((1u << lsp) - 1), k2 = (ee >> lsp) & (R - 1), pl = ee >> (lsp + t);
        const uint32_t cc = (pl << lsp) + ql, c = c0 + cc;
        const uint32_t q = c & ((1u << ls) - 1), p = c >> ls;
        const uint32_t k = t ? __brev(k2) >> (32 - t) : 0u;
        F v;
        tile_get(v, tile, (vl << le) | (k << lc) | cc);
        if (b.p.post_col) {   // last pass: p = 0, the output index is q + s k2
            F f;
            rec_load(f, b.p.post_row, k2);
            fp_mul(v, v, f);
            rec_load(f, b.p.post_col, q);
            fp_mul(v, v, f);
        } else if (b.p.has_scale) {
            fp_mul(v, v, scale);
        }
        if (b.p.out_plain) fp_from_mont(v, v);
        rec_store(b.p.out, (size_t)vec * b.out_stride + q + ((((size_t)p << t) + k2) << ls), v);
    }
}

// ---- h[idx[k]] += c[k]: the few terms of a constant times Z, added to a coefficient vector -----------------------------
__global__ void __launch_bounds__(64) k_fr_add_terms(const fr_terms a, uint32_t* h) {
    const int k = (int)threadIdx.x;
    if (k >= a.count) return;
    F x, c;
    rec_copy(c, a.c[k]);
    if (k == 0 && a.set) {
        x = c;
    } else {
        rec_load(x, h, a.idx[k]);
        fp_add(x, x, c);
    }
    rec_store(h, a.idx[k], x);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void l_pass(hipStream_t st, const fr_pass& a) {
    const unsigned tiles = 1u << (a.log_n - a.log_r - a.log_c);
    hipLaunchKernelGGL(k_fr_fft_pass, dim3(tiles), dim3(TPB), 0, st, a);
}

void l_powers(hipStream_t st, const uint32_t* table, const uint32_t* first, int out_plain, size_t n, uint32_t* d_out) {
    if (!n) return;
    fr_pow_args a;
    for (int b = 0; b < FR_POW_TABLE; ++b)
        for (int w = 0; w < N; ++w) a.table[b][w] = table[(size_t)b * N + w];
    for (int w = 0; w < N; ++w) a.first[w] = first ? first[w] : FR::R[w];
    int log_p = 8;   // one workgroup at the least, 2^16 lanes at the most
    while (log_p < FR_POW_TABLE - 1 && ((size_t)1 << log_p) < n) ++log_p;
    hipLaunchKernelGGL(k_fr_powers, dim3(1u << (log_p - 8)), dim3(TPB), 0, st, a, log_p, out_plain, n, d_out);
}

void l_muladd(hipStream_t st, size_t n, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, const uint32_t* k,
              int plain, uint32_t* d_out) {
    if (!n) return;
    fr_rec_arg kk = {};
    if (k)
        for (int w = 0; w < N; ++w) kk.v[w] = k[w];
    const size_t blocks = (n + TPB - 1) / TPB;
    hipLaunchKernelGGL(k_fr_muladd, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(TPB), 0, st, n, d_a, d_b, d_c, kk,
                       k ? 1 : 0, plain, d_out);
}

void l_lincomb(hipStream_t st, size_t n, int k, const uint32_t* const* d_v, const uint32_t* scalars, uint32_t* d_out) {
    if (!n) return;
    fr_lincomb_args a = {};
    for (int j = 0; j < k; ++j) {
        a.v[j] = d_v[j];
        for (int w = 0; w < N; ++w) a.s[j][w] = scalars[(size_t)j * N + w];
    }
    hipLaunchKernelGGL(k_fr_lincomb, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, n, k, a, d_out);
}

// ceil(batch / V) workgroups of whole vectors below 2^10 records, batch * n / 2^10 tiles from there on: a grid of at most
// 2^18 workgroups in x (batch * n <= 2^28)
void l_pass_batch(hipStream_t st, const fr_pass_batch& a) {
    const unsigned groups = ((a.batch + (1u << a.log_v) - 1) >> a.log_v) << a.log_tiles;
    hipLaunchKernelGGL(k_fr_fft_pass_batch, dim3(groups), dim3(TPB), 0, st, a);
}

void l_add_terms(hipStream_t st, const fr_terms& a, uint32_t* d_h) {
    if (a.count) hipLaunchKernelGGL(k_fr_add_terms, dim3(1), dim3(64), 0, st, a, d_h);
}

const fr_vtable g_frvt = {
    .curve = AMDMSM_FR_CURVE,
    .words = N,
    .two_adicity = FR::SQRT_S,
    .inv = FR::INV,
    .modulus = FR::P,
    .one = FR::R,
    .r2 = FR::R2,
    .root = FR::ROOT_OF_UNITY,
    .generator = FR::MULT_GENERATOR,
    .powers = l_powers,
    .pass = l_pass,
    .muladd = l_muladd,
    .lincomb = l_lincomb,
    .matrix_chunk = FRM_T,
    .matrix_apply = l_matrix_apply,
    .matrix_naive = l_matrix_naive,
    .scan = l_scan,
    .scan_naive = l_scan_naive,
    .domain_sweep = l_domain_sweep,
    .domain_combine = l_domain_combine,
    .domain_den = l_domain_den,
    .domain_divide = l_domain_divide,
    .domain_lagrange = l_domain_lagrange,
    .pass_batch = l_pass_batch,
    .add_terms = l_add_terms,
};

}  // namespace

const fr_vtable* AMDMSM_FR_VT() { return &g_frvt; }

}  // namespace amdmsm
