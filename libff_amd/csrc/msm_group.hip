// MSM kernels for ONE (curve, group) pair on gfx950.  Compiled once per group with
//   -DAMDMSM_GROUP=<traits struct from curve_params.h> -DAMDMSM_VT=<vtable getter>
// so the eight groups build in parallel and every modulus limb is a compile-time
// constant in the instruction stream.
//
// Pipeline (the device-side restatement of multi_exp_inner<BDLO12_signed>,
// multiexp.tcc:563-632, re-shaped for a throughput machine):
//   k_sort_*     signed radix-2^c recoding of every scalar (field_get_signed_digits,
//                field_utils.tcc:205-239) and a two-level LDS-staged bucket sort -> per-window
//                point lists grouped by bucket (k_count / k_scan / k_scatter: the global-atomic
//                fallback for c > 22)
//   k_accumulate one lane per S consecutive entries of a window's sorted list (segmented sum
//                by bucket, fixed work per lane): mixed additions
//                (multi_exp_add_element_to_bucket_with_signed_digit, multiexp.tcc:45-81) on
//                reduced-radix limbs (rr.cuh), records written as limbs; k_accumulate_fixup closes the
//                buckets that span lanes (its sums, like k_bucket_sums', stay on the limbs: rec_sum)
//   k_bucket_sums / k_plane_sums / k_window_horner
//                sum_b (b+1) * B_b (multiexp_accumulate_buckets, multiexp.tcc:90-125) as plain sums: row and
//                column sums of the weight matrix, bit planes, a short Horner per window (c >= 10;
//                k_reduce_segments / k_sum_butterfly -- running sums per segment -- below that)
//   k_horner     high-to-low window combination with c doublings (multiexp.tcc:612-629) on
//                lane-split field elements (wide.cuh)
//
// All windows are processed at once: the libff loop "for round ... signed_digits_round"
// becomes the W dimension of every grid.
#include "curve_params.h"
#include "ec.cuh"
#include "fp2h.cuh"
#include "group_vtable.h"
#include "wide.cuh"
#include "wide28.cuh"
#include "rr.cuh"

#include <algorithm>
#include <cstdio>
#include <vector>
#include <type_traits>

#ifndef AMDMSM_GROUP
#error "compile with -DAMDMSM_GROUP=<group traits> -DAMDMSM_VT=<vtable getter name>"
#endif

namespace amdmsm {
// the a x term of y^2 = x^3 + a x + b in the doublings of ec.cuh (0 but for the MNT groups; MNT4 G2: a' = 34 in Fq)
template <bool I>
struct ec_coeff_a<Fp<AMDMSM_GROUP::fq, I>> {
    static constexpr int value = AMDMSM_GROUP::DEG == 1 ? AMDMSM_GROUP::COEFF_A : 0;
};
template <int NR, bool I>
struct ec_coeff_a<Fp2<AMDMSM_GROUP::fq, NR, I>> {
    static constexpr int value = AMDMSM_GROUP::DEG == 2 ? AMDMSM_GROUP::COEFF_A : 0;
};
namespace {

using GP = AMDMSM_GROUP;
using FQ = typename GP::fq;
using FR = typename GP::fr;
static_assert(GP::COEFF_A == 0 || (!GP::HAS_ENDO && (GP::SUBGROUP_CHECK == 0 || GP::SUBGROUP_CHECK == 1) && GP::LIBFF_PROJECTIVE),
              "a != 0 is implemented for the MNT groups: no endomorphism, no subgroup test or [r]P == 0 on the plain "
              "Jacobian ladder (the endomorphism and reduced-radix tests are a = 0 only), projective records");
#if AMDMSM_ACC_RR || AMDMSM_ACC_SPLIT
static_assert(GP::COEFF_A == 0, "the reduced-radix and lane-pair accumulation loops are written for a = 0");
#endif

// Montgomery products are emitted inline only where AMDMSM_HOT_INLINE asks for it (the
// bucket-accumulation loop of narrow fields); everywhere else they are calls to one
// out-of-line copy per translation unit (fp.cuh, Fp<P, INL>).
#ifndef AMDMSM_HOT_INLINE
#define AMDMSM_HOT_INLINE 0
#endif
#ifndef AMDMSM_BENCH_BOTH
#define AMDMSM_BENCH_BOTH 0
#endif
// k_accumulate on almost-reduced coordinates (fp.cuh): no conditional subtraction after a
// product, an Fq2 product as two fused sums of two Fq products and Y3 as one fused sum (one
// Montgomery reduction each); 2-16 % faster on every group
#ifndef AMDMSM_ACC_LAZY
#define AMDMSM_ACC_LAZY 1
#endif
// minimum waves per SIMD the bucket-accumulation kernel is compiled for (register budget:
// 512 / waves, in granules of 8)
#ifndef AMDMSM_ACC_WAVES
#define AMDMSM_ACC_WAVES 1
#endif
// Overlap mode (engine.cpp amdmsm_ctx::bulk_stream): AMDMSM_OVERLAP_OK marks a group whose accumulation may be launched
// one workgroup per CU short of full occupancy (group_vtable::accumulate_overlap_ok, where ACC_OVERLAP_LDS is nonzero
// too).  It says nothing about the tail kernels' registers any more: no group caps them, and AMDMSM_TAIL_WAVES -- their
// minimum waves per SIMD -- stays at 1 unless an experiment build sets it.
#ifndef AMDMSM_OVERLAP_OK
#define AMDMSM_OVERLAP_OK 0
#endif
#ifndef AMDMSM_TAIL_WAVES
#define AMDMSM_TAIL_WAVES 1
#endif
template <int DEG, bool I> struct coord_sel;
template <bool I> struct coord_sel<1, I> { using type = Fp<FQ, I>; };
template <bool I> struct coord_sel<2, I> { using type = Fp2<FQ, GP::NR_SMALL == 0 ? -1 : GP::NR_SMALL, I>; };
#ifndef AMDMSM_COLD_INLINE
#define AMDMSM_COLD_INLINE 0
#endif
using E = typename coord_sel<GP::DEG, (AMDMSM_COLD_INLINE != 0)>::type;   // cold kernels
using EH = typename coord_sel<GP::DEG, (AMDMSM_HOT_INLINE != 0)>::type;  // k_accumulate
using EI = typename coord_sel<GP::DEG, true>::type;                      // probes only
// AMDMSM_ACC_SPLIT (G2 groups): k_accumulate keeps every Fq2 element split over a pair of lanes
// (fp2h.cuh) -- two physical lanes per accumulation lane, half the registers each
#ifndef AMDMSM_ACC_SPLIT
#define AMDMSM_ACC_SPLIT 0
#endif
template <int DEG> struct split_sel { using type = EH; static constexpr int LANES = 1; };
#if AMDMSM_ACC_SPLIT
template <> struct split_sel<2> { using type = Fp2H<FQ, (GP::NR_SMALL == 0 ? -1 : GP::NR_SMALL)>; static constexpr int LANES = 2; };
#endif
using EA = typename split_sel<GP::DEG>::type;            // element type of the accumulation loop
constexpr int ACC_LANES = split_sel<GP::DEG>::LANES;     // physical lanes per accumulation lane
// the bucket reduction (k_reduce_segments, k_sum_butterfly) uses the same split form: a wave then
// folds 32 segments instead of 64
using ER = typename std::conditional<(ACC_LANES == 2), EA, E>::type;
constexpr int RED_LANES = ACC_LANES;
constexpr uint32_t RED_FOLD = 64u / RED_LANES;
#if AMDMSM_ACC_RR
static_assert(GP::DEG == 1 || AMDMSM_ACC_SPLIT, "reduced-radix Fq2 accumulation works on lane pairs");
template <int DEG> struct rr_el_sel { using type = Rr<FQ>; };
template <> struct rr_el_sel<2> { using type = Rr2H<FQ, (GP::NR_SMALL == 0 ? -1 : GP::NR_SMALL)>; };
using ERR = typename rr_el_sel<GP::DEG>::type;   // element type of the reduced-radix accumulation loop
#endif

constexpr int EW = FQ::N * GP::DEG;   // words per coordinate
constexpr int AFFW = 2 * EW;          // words per compact affine point
constexpr int XYZW = 3 * EW;          // words per (X, Y, Z) record
constexpr int ZZW = 4 * EW;           // words per (X, Y, ZZ, ZZZ) bucket accumulator
// AMDMSM_ACC_RR: k_accumulate keeps its accumulators on reduced-radix limbs (rr.cuh; an Fq2 element over a pair of
// lanes as with AMDMSM_ACC_SPLIT) and writes them as they are -- 4 L limbs per component; the kernels that read the
// records take that form or canonical (X, Y, ZZ, ZZZ) words (load_xyzz_rec / rec_load_rho).  ZZS = words between two
// records of the bucket / partial arrays (group_vtable::bucket_words).
#ifndef AMDMSM_ACC_RR
#define AMDMSM_ACC_RR 0
#endif
#if AMDMSM_ACC_RR
constexpr int RRL = rr_shape<FQ>::L;
constexpr int ZZS = 4 * RRL * GP::DEG;   // [component][X, Y, ZZ, ZZZ][limb]: a lane's 4 L limbs are contiguous
#else
constexpr int ZZS = ZZW;
#endif
constexpr int FRW = FR::N;            // words per scalar
constexpr int TPB = 256;

AMDMSM_DEV size_t gtid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
AMDMSM_DEV uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

template <class T> AMDMSM_DEV void load_aff(Aff<T>& p, const uint32_t* q) {
    el_load(p.x, q);
    el_load(p.y, q + EW);
}
template <class T> AMDMSM_DEV void store_aff(uint32_t* q, const Aff<T>& p) {
    el_store(q, p.x);
    el_store(q + EW, p.y);
}
template <class T> AMDMSM_DEV void load_jac(Jac<T>& p, const uint32_t* q) {
    el_load(p.x, q);
    el_load(p.y, q + EW);
    el_load(p.z, q + 2 * EW);
}
template <class T> AMDMSM_DEV void store_jac(uint32_t* q, const Jac<T>& p) {
    el_store(q, p.x);
    el_store(q + EW, p.y);
    el_store(q + 2 * EW, p.z);
}
template <class T> AMDMSM_DEV void load_xyzz(Xyzz<T>& p, const uint32_t* q) {
    el_load(p.x, q);
    el_load(p.y, q + EW);
    el_load(p.zz, q + 2 * EW);
    el_load(p.zzz, q + 3 * EW);
}
template <class T> AMDMSM_DEV void store_xyzz(uint32_t* q, const Xyzz<T>& p) {
    el_store(q, p.x);
    el_store(q + EW, p.y);
    el_store(q + 2 * EW, p.zz);
    el_store(q + 3 * EW, p.zzz);
}

// libff in-memory record -> engine Jacobian
AMDMSM_DEV void load_libff(Jac<E>& p, const uint32_t* q) {
    load_jac(p, q);
    if (GP::LIBFF_PROJECTIVE) {
        // (X : Y : Z) homogeneous, x = X/Z, y = Y/Z  ->  Jacobian (X*Z, Y*Z^2, Z)
        if (el_is_zero(p.z)) {
            jac_set_inf(p);
        } else {
            E zz;
            el_sqr(zz, p.z);
            el_mul(p.x, p.x, p.z);
            el_mul(p.y, p.y, zz);
        }
    }
}

// engine Jacobian -> requested output convention
AMDMSM_DEV void store_out(uint32_t* q, const Jac<E>& p, int form) {
    Jac<E> o;
    if (form == OUT_JACOBIAN) {
        o = p;
    } else if (jac_is_inf(p)) {
        jac_set_inf(o);   // libff zero = (0, 1, 0) in every coordinate system used here
    } else if (form == OUT_AFFINE) {
        Aff<E> a;
        jac_to_aff(a, p);
        o.x = a.x;
        o.y = a.y;
        el_one(o.z);
    } else if (GP::LIBFF_PROJECTIVE) {
        // Jacobian (X, Y, Z): x = X/Z^2, y = Y/Z^3  ->  homogeneous (X*Z : Y : Z^3)
        E zz;
        el_sqr(zz, p.z);
        el_mul(o.x, p.x, p.z);
        o.y = p.y;
        el_mul(o.z, zz, p.z);
    } else {
        o = p;
    }
    store_jac(q, o);
}

// ---------------------------------------------------------------- recoding
// Signed radix-2^c digits, least-significant window first, exactly
// field_get_signed_digits (field_utils.tcc:205-239): digit = raw + carry;
// overflow (digit == 2^c) -> 0 with carry; bit c-1 set -> digit - 2^c with carry.
// The scalar is streamed through a 64-bit bit buffer so no private array is
// indexed at run time (which would send it to scratch).
template <int NW, class F>
AMDMSM_DEV void for_each_signed_digit(const uint32_t (&s)[NW], int c, int W, F&& emit) {
    const uint32_t mask = (1u << c) - 1u;
    uint64_t buf = 0;
    int nbits = 0;
    int w = 0;
    uint32_t carry = 0;
    auto step = [&](uint32_t raw) {
        const uint32_t digit = raw + carry;
        const uint32_t overflow = (digit >> c) & 1u;
        const uint32_t cbit = (digit >> (c - 1)) & 1u;
        const int32_t d = overflow ? 0 : (int32_t)digit - (int32_t)(cbit << c);
        carry = overflow | cbit;
        emit(w, d);
        ++w;
    };
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        buf |= (uint64_t)s[j] << nbits;
        nbits += 32;
        while (nbits >= c && w < W) {
            step((uint32_t)buf & mask);
            buf >>= c;
            nbits -= c;
        }
    }
    while (w < W) {
        step((uint32_t)buf & mask);
        buf >>= c;
    }
}

AMDMSM_DEV void load_scalar(uint32_t (&s)[FRW], const uint32_t* scalars, size_t i, int mont) {
    Fp<FR> x;
    fp_load(x, scalars + i * FRW);
    if (mont) fp_from_mont(x, x);   // Fp_model::as_bigint, multiexp.tcc:579-582
#pragma unroll
    for (int j = 0; j < FRW; ++j) s[j] = x.v[j];
}

// ---------------------------------------------------------------- endomorphism split
// k = k1 + k2 lambda (mod r) with |k1|, |k2| <= GLV::BOUND ~ sqrt(r) (constants and their
// derivation: tools/gen_params.py glv_params; phi(x, y) = (beta x, y) = [lambda](x, y) on the
// order-r subgroup).  The MSM over n points with Fr::num_bits-bit scalars becomes one over the 2n
// points P_i, phi(P_i) with half-length scalars: same number of bucket entries, half the windows.
using GLV = typename GP::glv;
constexpr int GLV_HW = GLV::HW;       // limbs of |k1|, |k2|
constexpr int GLV_HC = GLV::HW + 1;   // working width: two's complement with room for the sign

// The schoolbook products below gather one 32-bit column at a time in a 96-bit accumulator (lo: 64, hi: 32) on the
// carry chains of fp.cuh (mac_chain.inc): one v_mad_u64_u32 and one carry add per product, the per-lane operand in a
// VGPR and the constant limb in an SGPR.  The constants are picked at compile time -- SEL 0 / 1: G1 / G2, 2 .. 5:
// M[0] .. M[3] -- and their zero top limbs are left out of the chains.
template <int SEL>
constexpr uint32_t glv_const(int j) {
    return SEL == 0 ? GLV::G1[j] : SEL == 1 ? GLV::G2[j] : GLV::M[SEL - 2][j];
}
template <int SEL>
constexpr int glv_const_width() {   // limbs up to the highest nonzero one
    int w = 0;
    for (int j = 0; j < (SEL < 2 ? GLV::GW : GLV_HC); ++j)
        if (glv_const<SEL>(j) != 0) w = j + 1;
    return w;
}
// acc += sum_{i in [I0, I0 + CNT)} a[i] * const[K - i]
template <int SEL, int K, int I0, size_t... J>
AMDMSM_DEV void glv_mac_col(uint64_t& lo, uint32_t& hi, const uint32_t* a, std::index_sequence<J...>) {
    mac_chain<(int)sizeof...(J)>::vs(lo, hi, a[I0 + (int)J]...,
                                     std::integral_constant<uint32_t, glv_const<SEL>(K - I0 - (int)J)>::value...);
}
// i runs over [LO, HI) cut to the limbs the constant has: chunks of at most MAC_CHUNK products
template <int SEL, int K, int LO, int HI>
AMDMSM_DEV void glv_mac_range(uint64_t& lo, uint32_t& hi, const uint32_t* a) {
    constexpr int L = K - glv_const_width<SEL>() + 1 > LO ? K - glv_const_width<SEL>() + 1 : LO;
    if constexpr (L < HI) {
        constexpr int CNT = (HI - L) < MAC_CHUNK ? (HI - L) : MAC_CHUNK;
        glv_mac_col<SEL, K, L>(lo, hi, a, std::make_index_sequence<CNT>{});
        glv_mac_range<SEL, K, L + CNT, HI>(lo, hi, a);
    }
}
AMDMSM_DEV uint32_t glv_next_column(uint64_t& lo, uint32_t& hi) {   // emit the low word, shift down by one word
    const uint32_t w = (uint32_t)lo;
    lo = (lo >> 32) | ((uint64_t)hi << 32);
    hi = 0;
    return w;
}
// (A 32-bit word added at the start of a column needs no carry: the accumulator is then the shifted-down rest of the
// column before, whose top word counted that column's carries -- far below 2^63.)
// low GLV_HC limbs of (k G + 2^(s-1)) >> s, s = 32 (FRW + 1): Babai rounding of k b / r
template <int SEL, int COL>
AMDMSM_DEV void glv_round_col(uint64_t& lo, uint32_t& hi, uint32_t (&c)[GLV_HC], const uint32_t* k) {
    if constexpr (COL == FRW) lo += 0x80000000u;
    glv_mac_range<SEL, COL, 0, (COL < FRW ? COL + 1 : FRW)>(lo, hi, k);
    const uint32_t w = glv_next_column(lo, hi);
    if constexpr (COL >= FRW + 1) c[COL - FRW - 1] = w;
    if constexpr (COL + 1 < FRW + 1 + GLV_HC) glv_round_col<SEL, COL + 1>(lo, hi, c, k);
}
template <int SEL>
AMDMSM_DEV void glv_round_mul(uint32_t (&c)[GLV_HC], const uint32_t (&k)[FRW]) {
    uint64_t lo = 0;
    uint32_t hi = 0;
    glv_round_col<SEL, 0>(lo, hi, c, k);
}
// t = k (if ADD_K) + c1 * A + c2 * B  mod 2^(32 GLV_HC), A = M[SA], B = M[SA + 1]
template <bool ADD_K, int SA, int COL>
AMDMSM_DEV void glv_combine_col(uint64_t& lo, uint32_t& hi, uint32_t (&t)[GLV_HC], const uint32_t (&k)[FRW], const uint32_t* c1,
                                const uint32_t* c2) {
    if constexpr (ADD_K && COL < FRW) lo += k[COL];
    glv_mac_range<2 + SA, COL, 0, COL + 1>(lo, hi, c1);
    glv_mac_range<3 + SA, COL, 0, COL + 1>(lo, hi, c2);
    t[COL] = glv_next_column(lo, hi);
    if constexpr (COL + 1 < GLV_HC) glv_combine_col<ADD_K, SA, COL + 1>(lo, hi, t, k, c1, c2);
}
template <bool ADD_K, int SA>
AMDMSM_DEV void glv_combine(uint32_t (&t)[GLV_HC], const uint32_t (&k)[FRW], const uint32_t (&c1)[GLV_HC],
                            const uint32_t (&c2)[GLV_HC]) {
    uint64_t lo = 0;
    uint32_t hi = 0;
    glv_combine_col<ADD_K, SA, 0>(lo, hi, t, k, c1, c2);
}
// two's complement t -> (|t|, sign)
AMDMSM_DEV bool glv_magnitude(uint32_t (&m)[GLV_HW], const uint32_t (&t)[GLV_HC]) {
    const bool neg = (t[GLV_HC - 1] >> 31) != 0;
    uint32_t carry = neg ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < GLV_HW; ++i) {
        const uint32_t v = neg ? ~t[i] : t[i];
        m[i] = v + carry;
        carry = (m[i] < v) ? 1u : 0u;
    }
    return neg;
}
AMDMSM_DEV void glv_split(const uint32_t (&k)[FRW], uint32_t (&m1)[GLV_HW], bool& neg1, uint32_t (&m2)[GLV_HW], bool& neg2) {
    uint32_t c1[GLV_HC], c2[GLV_HC], t[GLV_HC];
    glv_round_mul<0>(c1, k);
    glv_round_mul<1>(c2, k);
    glv_combine<true, 0>(t, k, c1, c2);
    neg1 = glv_magnitude(m1, t);
    glv_combine<false, 2>(t, k, c1, c2);
    neg2 = glv_magnitude(m2, t);
}
// the two halves of scalar i, recoded: emit(half, w, d) -- half 0 belongs to P_i, half 1 to phi(P_i)
template <class F>
AMDMSM_DEV void for_each_glv_digit(const uint32_t (&k)[FRW], int c, int W, F&& emit) {
    uint32_t m1[GLV_HW], m2[GLV_HW];
    bool n1, n2;
    glv_split(k, m1, n1, m2, n2);
    for_each_signed_digit(m1, c, W, [&](int w, int32_t d) { emit(0, w, n1 ? -d : d); });
    for_each_signed_digit(m2, c, W, [&](int w, int32_t d) { emit(1, w, n2 ? -d : d); });
}

// Histogram / cursor updates with wave-level aggregation of hot keys.  With uniformly random
// digits the 64 lanes of a wave hit 64 different counters and every lane issues its own
// atomic (the loop below exits after one cheap probe).  Skewed inputs -- the short top
// window whose few buckets receive every point, witness vectors full of 0/1 scalars -- put
// most lanes on one counter; then the lanes that share the first active lane's key are
// served by ONE atomic (count) or one atomic plus a lane rank (scatter), round after round,
// until the leading key is rare again.  Must be called by every lane of the wave.
constexpr int HOT_KEY_MIN = 8;

template <bool WANT_POS>
AMDMSM_DEV uint32_t wave_key_add(uint32_t* __restrict__ ctr, uint32_t key, bool active) {
    uint32_t pos = 0;
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        const unsigned long long m = __ballot(active);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader, 64);
        const unsigned long long same = __ballot(active && key == k0);
        const int cnt = __popcll(same);
        if (cnt < HOT_KEY_MIN) break;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(&ctr[k0], (uint32_t)cnt);
        if (WANT_POS) {
            base = (uint32_t)__shfl((int)base, leader, 64);
            if (active && key == k0) pos = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        }
        active = active && key != k0;
    }
    if (active) pos = atomicAdd(&ctr[key], 1u);
    return pos;
}

__global__ void __launch_bounds__(TPB) k_count(const uint32_t* __restrict__ scalars, size_t n, int mont, int c, int W,
                                               uint32_t* __restrict__ counts) {
    const size_t i = gtid();
    const bool live = i < n;
    uint32_t s[FRW];
    if (live) {
        load_scalar(s, scalars, i, mont);
    } else {
#pragma unroll
        for (int j = 0; j < FRW; ++j) s[j] = 0;   // recodes to all-zero digits
    }
    const size_t B = (size_t)1 << (c - 1);
    for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
        const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
        wave_key_add<false>(counts + (size_t)w * B, idx, d != 0);
    });
}

__global__ void __launch_bounds__(TPB) k_scatter(const uint32_t* __restrict__ scalars, size_t n, int mont, int c, int W,
                                                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ lists,
                                                 size_t list_stride) {
    const size_t i = gtid();
    const bool live = i < n;
    uint32_t s[FRW];
    if (live) {
        load_scalar(s, scalars, i, mont);
    } else {
#pragma unroll
        for (int j = 0; j < FRW; ++j) s[j] = 0;
    }
    const size_t B = (size_t)1 << (c - 1);
    for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
        const uint32_t neg = d < 0 ? 1u : 0u;
        const uint32_t idx = (uint32_t)(neg ? -d : d) - 1u;
        const uint32_t pos = wave_key_add<true>(cursor + (size_t)w * B, idx, d != 0);
        if (d != 0) lists[(size_t)w * list_stride + pos] = (uint32_t)i | (neg << 31);
    });
}

__global__ void __launch_bounds__(TPB) k_digits(const uint32_t* __restrict__ scalars, size_t n, int mont, int c, int W,
                                                int32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    uint32_t s[FRW];
    load_scalar(s, scalars, i, mont);
    for_each_signed_digit(s, c, W, [&](int w, int32_t d) { out[i * (size_t)W + w] = d; });
}

// test hook: out[(2 i + half) * W + w] = digit w of half `half` of scalar i
__global__ void __launch_bounds__(TPB) k_glv_digits(const uint32_t* __restrict__ scalars, size_t n, int mont, int c, int W,
                                                    int32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    uint32_t s[FRW];
    load_scalar(s, scalars, i, mont);
    for_each_glv_digit(s, c, W, [&](int h, int w, int32_t d) { out[(2 * i + h) * (size_t)W + w] = d; });
}
// phi(P_i) = (beta x_i, y_i) as compact affine records of their own (so that the accumulation
// loop reads either kind of point as one contiguous record): one thread per Fq component
__global__ void __launch_bounds__(TPB) k_endo_points(const uint32_t* __restrict__ bases, size_t n, uint32_t* __restrict__ out) {
    const size_t t = gtid();
    if (t >= n * 2 * GP::DEG) return;
    const bool is_x = (t % (2 * GP::DEG)) < (size_t)GP::DEG;
    Fp<FQ> v, beta;
    fp_load(v, bases + t * FQ::N);
    if (is_x) {
#pragma unroll
        for (int j = 0; j < FQ::N; ++j) beta.v[j] = GP::GLV_BETA[j];
        fp_mul(v, v, beta);
    }
    fp_store(out + t * FQ::N, v);
}

// multi_exp_filter_one_zero's classification (multiexp.tcc:713-733: is_zero(), == FieldT::one())
// as two device counters; one global atomic per wave and class.
__global__ void __launch_bounds__(TPB) k_scalar_stats(const uint32_t* __restrict__ scalars, size_t n, int mont,
                                                      uint32_t* __restrict__ stats) {
    uint32_t zeros = 0, ones = 0;
    for (size_t i = gtid(); i < n; i += (size_t)gridDim.x * TPB) {
        Fp<FR> x, one;
        fp_load(x, scalars + i * FRW);
        if (mont) {
            fp_set_one(one);
        } else {
            fp_set_zero(one);
            one.v[0] = 1u;
        }
        zeros += fp_is_zero(x) ? 1u : 0u;
        ones += fp_eq(x, one) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        zeros += (uint32_t)__shfl_xor((int)zeros, off, 64);
        ones += (uint32_t)__shfl_xor((int)ones, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (zeros) atomicAdd(&stats[0], zeros);
        if (ones) atomicAdd(&stats[1], ones);
    }
}

// Exclusive scan of one window's histogram per workgroup (grid.x = W).
constexpr int SCAN_TPB = 1024;
constexpr int SCAN_ITEMS = 4;
__global__ void __launch_bounds__(SCAN_TPB) k_scan(uint32_t* __restrict__ counts, uint32_t B) {
    __shared__ uint32_t wave_sums[SCAN_TPB / 64];
    __shared__ uint32_t running;
    uint32_t* p = counts + (size_t)blockIdx.x * B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (uint32_t base = 0; base < B; base += SCAN_TPB * SCAN_ITEMS) {
        const uint32_t i0 = base + threadIdx.x * SCAN_ITEMS;
        uint32_t v[SCAN_ITEMS];
        uint32_t tsum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            v[k] = (i0 + k < B) ? p[i0 + k] : 0u;
            tsum += v[k];
        }
        // inclusive scan of per-thread sums inside the wave
        uint32_t inc = tsum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        if (lane == 63) wave_sums[wave] = inc;
        __syncthreads();
        uint32_t wave_off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_TPB / 64; ++k) {
            const uint32_t ws = wave_sums[k];
            if (k < wave) wave_off += ws;
            total += ws;
        }
        uint32_t excl = running + wave_off + inc - tsum;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (i0 + k < B) p[i0 + k] = excl;
            excl += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) running += total;
        __syncthreads();
    }
}

// ------------------------------------------------- LDS-staged two-level sort
// Grouping the n*W (point, window) entries by bucket with one global atomic and one scattered
// 4-byte store per entry (k_count / k_scatter above) runs at the L2 atomic rate (~25 G/s) and
// is half of a 2^26-point MSM.  This path keeps the atomics in LDS and makes every global write
// a run of neighbouring entries:
//   k_sort_digits   one pass over the scalars: signed digits to digits[w][i] (coalesced) and a
//                   histogram over the top HB bits of the bucket index ("coarse bin"), per
//                   workgroup in LDS, merged with one global atomic per (workgroup, bin)
//   k_sort_coarse   workgroup (tile, w): exclusive scan of the window's coarse histogram (2^HB counts),
//                   LDS counting sort of a tile's nonzero digits by coarse bin, one global atomic
//                   per (tile, bin) to reserve space, runs written to tmp[w] as (payload, fine
//                   key) pairs
//   k_sort_fine     workgroup (bin, w): LDS histogram of the bin by the low FB bits -> ends[],
//                   then chunk-wise LDS counting sort -> lists[w] (runs per fine bucket)
// bucket index = |digit| - 1 = (coarse << FB) | fine, HB = min(10, c-1), FB = c-1-HB.
constexpr int SORT_TPB = (int)SORT_DIGIT_TPB;   // 1024 (group_vtable.h, beside the digit pass's grid rule)
#ifndef AMDMSM_SORT_TILE
#define AMDMSM_SORT_TILE 16384
#endif
#ifndef AMDMSM_SORT_KEY32
#define AMDMSM_SORT_KEY32 0
#endif
#if AMDMSM_SORT_KEY32
using sort_key_t = uint32_t;
#else
using sort_key_t = unsigned short;   // fine part of the bucket index between the two sort levels
#endif
constexpr int SORT_TILE = AMDMSM_SORT_TILE;    // entries per k_sort_coarse workgroup
constexpr int SORT_CHUNK = 16384;   // entries per k_sort_fine chunk
constexpr int SORT_MAX_HB = 10;
constexpr int SORT_MAX_FB = 11;     // c <= 22

AMDMSM_DEV uint32_t digit_payload(size_t i, int32_t d) { return (uint32_t)i | (d < 0 ? 0x80000000u : 0u); }

// exclusive scan of cnt[0..len) (LDS) into out[0..len) by one workgroup of NT threads;
// len <= MP * NT (MP: entries per thread, 8 unless the caller knows better and wants the registers).  tmp: NT/64 + 1
// words of LDS.  Returns the total in every thread.
template <int NT = SORT_TPB, int MP = 8>
AMDMSM_DEV uint32_t block_exclusive_scan(const uint32_t* cnt, uint32_t* out, uint32_t len, uint32_t* tmp) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (len + NT - 1) / NT;   // <= MP
    const uint32_t i0 = tid * per;
    uint32_t v[MP];
    uint32_t tsum = 0;
#pragma unroll
    for (uint32_t k = 0; k < MP; ++k) {
        v[k] = (k < per && i0 + k < len) ? cnt[i0 + k] : 0u;
        tsum += v[k];
    }
    uint32_t inc = tsum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
        if ((int)lane >= off) inc += o;
    }
    __syncthreads();   // protect tmp / out reuse
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    uint32_t wave_off = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < NT / 64; ++k) {
        const uint32_t ws = tmp[k];
        if (k < wave) wave_off += ws;
        total += ws;
    }
    uint32_t excl = wave_off + inc - tsum;
#pragma unroll
    for (uint32_t k = 0; k < MP; ++k) {
        if (k < per && i0 + k < len) out[i0 + k] = excl;
        excl += v[k];
    }
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(SORT_TPB) k_sort_digits(const uint32_t* __restrict__ scalars, size_t n, int mont, int c,
                                                          int W, int hb, int32_t* __restrict__ digits,
                                                          size_t stride, uint32_t* __restrict__ coarse_counts, int mode,
                                                          int dtop) {
    // mode 1 (flat): the W digits of scalar i are entries i*W .. i*W+W-1 of ONE list (they index a
    // table of precomputed multiples [2^(jc)]P_i and share a single bucket set)
    // mode 2 (endomorphism): scalar i gives two columns of W digits, i (k1, for P_i) and n + i
    // (k2, for phi(P_i))
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];   // [W][2^hb]   (flat: [2^hb])
    const bool flat = mode == 1;
    const uint32_t nbin = 1u << hb;
    const int fb = c - 1 - hb, fbt = fb - dtop;   // fine bits; those of the top window (sort_top_shift; dtop = 0 when flat)
    const uint32_t nctr = flat ? nbin : (uint32_t)W * nbin;
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) smem[j] = 0;
    __syncthreads();
    // blocks blockIdx.x, blockIdx.x + gridDim.x, ... of SORT_TPB scalars (group_vtable.h sort_digit_grid), one histogram
    const size_t nblocks = (n + SORT_TPB - 1) / SORT_TPB;
    for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const size_t i = blk * SORT_TPB + threadIdx.x;
        if (i >= n) break;
        uint32_t s[FRW];
        load_scalar(s, scalars, i, mont);
        if (mode == 2) {
            for_each_glv_digit(s, c, W, [&](int h, int w, int32_t d) {
                digits[(size_t)w * stride + (h ? n + i : i)] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(uint32_t)w * nbin + (idx >> (w == W - 1 ? fbt : fb))], 1u);
                }
            });
        } else {
            for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
                digits[flat ? i * (size_t)W + w : (size_t)w * stride + i] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(flat ? 0u : (uint32_t)w * nbin) + (idx >> (w == W - 1 ? fbt : fb))], 1u);
                }
            });
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) {
        const uint32_t v = smem[j];
        if (v) atomicAdd(&coarse_counts[(j / nbin) * (nbin + 1) + (j % nbin)], v);
    }
}

// Scalar selection (amdmsm_*_batch_items): the scalar of base i comes from a vector shared by several MSMs --
// element index[i] of it (index list: any order, repeats allowed) or element offset + i (slice).  Only the load is
// redirected; digit columns and payloads stay indexed by the base i.  An element at or past shared_n is never
// dereferenced: it counts as scalar 0 and raises *flag, which the engine turns into AMDMSM_ERR_BAD_ARG.
// Every lane still loads one whole scalar with 16-byte (10-word fields: 8-byte) loads, as the streaming form does.
using scalar_sel = sort_src::selection;
AMDMSM_DEV void load_scalar_sel(uint32_t (&s)[FRW], const uint32_t* shared, const scalar_sel& sel, size_t i, int mont) {
    const size_t idx = sel.index ? (size_t)sel.index[i] : sel.offset + i;
    if (idx >= sel.shared_n) {
#pragma unroll
        for (int j = 0; j < FRW; ++j) s[j] = 0;
        atomicOr(sel.flag, 1u);
        return;
    }
    load_scalar(s, shared, idx, mont);
}

// k_sort_digits with the selecting load.  A kernel of its own, body and all: sharing the body with k_sort_digits through
// a template changed that kernel's register allocation, and the code of the existing call paths is to stay as it is.
__global__ void __launch_bounds__(SORT_TPB) k_sort_digits_sel(const uint32_t* __restrict__ shared, size_t n, int mont, int c,
                                                              int W, int hb, int32_t* __restrict__ digits,
                                                              size_t stride, uint32_t* __restrict__ coarse_counts, int mode,
                                                              const uint32_t* __restrict__ index, size_t offset,
                                                              size_t shared_n, uint32_t* __restrict__ flag, int dtop) {
    const scalar_sel sel{index, offset, shared_n, flag};
    // mode 1 (flat): the W digits of scalar i are entries i*W .. i*W+W-1 of ONE list (they index a
    // table of precomputed multiples [2^(jc)]P_i and share a single bucket set)
    // mode 2 (endomorphism): scalar i gives two columns of W digits, i (k1, for P_i) and n + i
    // (k2, for phi(P_i))
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];   // [W][2^hb]   (flat: [2^hb])
    const bool flat = mode == 1;
    const uint32_t nbin = 1u << hb;
    const int fb = c - 1 - hb, fbt = fb - dtop;   // fine bits; those of the top window (sort_top_shift; dtop = 0 when flat)
    const uint32_t nctr = flat ? nbin : (uint32_t)W * nbin;
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) smem[j] = 0;
    __syncthreads();
    // blocks blockIdx.x, blockIdx.x + gridDim.x, ... of SORT_TPB scalars (group_vtable.h sort_digit_grid), one histogram
    const size_t nblocks = (n + SORT_TPB - 1) / SORT_TPB;
    for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const size_t i = blk * SORT_TPB + threadIdx.x;
        if (i >= n) break;
        uint32_t s[FRW];
        load_scalar_sel(s, shared, sel, i, mont);
        if (mode == 2) {
            for_each_glv_digit(s, c, W, [&](int h, int w, int32_t d) {
                digits[(size_t)w * stride + (h ? n + i : i)] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(uint32_t)w * nbin + (idx >> (w == W - 1 ? fbt : fb))], 1u);
                }
            });
        } else {
            for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
                digits[flat ? i * (size_t)W + w : (size_t)w * stride + i] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(flat ? 0u : (uint32_t)w * nbin) + (idx >> (w == W - 1 ? fbt : fb))], 1u);
                }
            });
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) {
        const uint32_t v = smem[j];
        if (v) atomicAdd(&coarse_counts[(j / nbin) * (nbin + 1) + (j % nbin)], v);
    }
}
// out[i] = the scalar base i selects (the one-after-the-other route of a batch outside the limits of one pass)
__global__ void __launch_bounds__(TPB) k_gather_scalars(const uint32_t* __restrict__ shared, size_t n,
                                                        const uint32_t* __restrict__ index, size_t offset, size_t shared_n,
                                                        uint32_t* __restrict__ flag, uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    uint32_t s[FRW];
    load_scalar_sel(s, shared, scalar_sel{index, offset, shared_n, flag}, i, 0);
    Fp<FR> x;
#pragma unroll
    for (int j = 0; j < FRW; ++j) x.v[j] = s[j];
    fp_store(out + i * FRW, x);
}

// ------------------------------------------------- scalars known to be short (amdmsm_*_short)
// KIND = AMDMSM_SCALAR_*: 0 = Fr records, otherwise the bytes of one packed little-endian unsigned integer (1, 2, 4, 8).
// Packed integers are read 16 bytes per lane -- 16 / 8 / 4 / 2 consecutive elements -- wherever the vector is 16-byte
// aligned; the pointer itself needs only the element's alignment, so up to 16 / WB - 1 elements in front of the first
// boundary ("head") and as many behind the last whole vector ("tail") are read one by one.  Work items of a pass:
// item t < nvec is the vector of elements head + t * EPL ..., item nvec + e is single element e of head and tail.
template <int WB>
struct packed_split {
    static constexpr int EPL = 16 / WB;
    size_t head, nvec, rest;   // rest = head + tail
    AMDMSM_HD packed_split(const void* p, size_t n) {
        const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(p) & 15u);
        head = mis ? (16 - mis) / WB : 0;
        if (head > n) head = n;
        nvec = (n - head) / EPL;
        rest = n - nvec * EPL;
    }
    AMDMSM_HD size_t items() const { return nvec + rest; }
    AMDMSM_HD size_t single_index(size_t t) const {
        const size_t e = t - nvec;
        return e < head ? e : nvec * EPL + e;
    }
};
template <int WB>
AMDMSM_DEV uint64_t packed_elem(const uint32_t (&v)[4], int j) {   // j is a constant after unrolling
    if (WB == 8) return (uint64_t)v[(2 * j) & 3] | ((uint64_t)v[(2 * j + 1) & 3] << 32);
    if (WB == 4) return v[j & 3];
    if (WB == 2) return (v[(j >> 1) & 3] >> (16 * (j & 1))) & 0xffffu;
    return (v[(j >> 2) & 3] >> (8 * (j & 3))) & 0xffu;
}
template <int WB>
AMDMSM_DEV uint64_t packed_one(const void* p, size_t i) {
    if (WB == 8) return reinterpret_cast<const uint64_t*>(p)[i];
    if (WB == 4) return reinterpret_cast<const uint32_t*>(p)[i];
    if (WB == 2) return reinterpret_cast<const unsigned short*>(p)[i];
    return reinterpret_cast<const unsigned char*>(p)[i];
}
AMDMSM_DEV void packed_vec(uint32_t (&v)[4], const void* p, size_t byte_off) {
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(p) + byte_off);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
}

// Bit length of the longest scalar: *out = max(*out, max_i bits(scalar i)); *out is cleared by the caller.
// Fr records are reduced first (load_scalar), packed integers are OR-ed together.  One atomic per wave.
template <int KIND>
__global__ void __launch_bounds__(TPB) k_scalar_bits(const void* __restrict__ scalars, size_t n, int mont,
                                                     uint32_t* __restrict__ out) {
    uint32_t top = 0;
    const size_t step = (size_t)gridDim.x * TPB;
    if constexpr (KIND == 0) {
        for (size_t i = gtid(); i < n; i += step) {
            uint32_t s[FRW];
            load_scalar(s, reinterpret_cast<const uint32_t*>(scalars), i, mont);
            uint32_t b = 0;
#pragma unroll
            for (int j = 0; j < FRW; ++j) {
                if (s[j]) b = 32u * j + 32u - (uint32_t)__clz((int)s[j]);
            }
            top = b > top ? b : top;
        }
    } else {
        const packed_split<KIND> sp(scalars, n);
        uint64_t acc = 0;
        for (size_t t = gtid(); t < sp.items(); t += step) {
            if (t < sp.nvec) {
                uint32_t v[4];
                packed_vec(v, scalars, (sp.head * KIND) + t * 16);
                acc |= (uint64_t)(v[0] | v[2]) | ((uint64_t)(v[1] | v[3]) << 32);
            } else {
                acc |= packed_one<KIND>(scalars, sp.single_index(t));
            }
        }
        if (KIND < 8) acc = (acc | (acc >> 32)) & 0xffffffffull;   // elements narrower than a word: fold the halves
        if (KIND == 2) acc = (acc | (acc >> 16)) & 0xffffull;
        if (KIND == 1) {
            acc |= acc >> 16;
            acc = (acc | (acc >> 8)) & 0xffull;
        }
        top = acc ? 64u - (uint32_t)__clzll((long long)acc) : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)top, off, 64);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(out, top);
}

// The digit pass of the two-level sort (k_sort_digits, mode 0) for scalars below 2^limit_bits: W covers limit_bits + 2
// bits only.  A kernel of its own, body and all, for the reason given above k_sort_digits_sel.
//   packed integers: the scalar is one or two words in registers; a lane recodes the 16 / 8 / 4 / 2 elements of its
//     16-byte load one after the other, so the digit columns a wave writes are one contiguous run per window
//   Fr records: reduced as usual; the words at and above limit_bits are known to be zero and W ends the recoding after
//     the digits the low ceil(limit_bits / 32) words fill
// A scalar with a bit at or above limit_bits (a broken promise) raises *flag and counts as 0; limit_bits at the
// kind's full width tests nothing and flag is not touched.
template <int KIND>
__global__ void __launch_bounds__(SORT_TPB) k_sort_digits_short(const void* __restrict__ scalars, size_t n, int mont, int c,
                                                                int W, int hb, uint32_t block, int32_t* __restrict__ digits,
                                                                size_t stride, uint32_t* __restrict__ coarse_counts,
                                                                int limit_bits, uint32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];   // [W][2^hb]
    const uint32_t nbin = 1u << hb;
    const int fb = c - 1 - hb;
    const uint32_t nctr = (uint32_t)W * nbin;
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) smem[j] = 0;
    __syncthreads();
    // blocks blockIdx.x, blockIdx.x + gridDim.x, ... of `block` <= SORT_TPB work items (group_vtable.h sort_digit_grid),
    // one histogram; the threads at and past `block` of a workgroup only help to clear and to merge it
    if constexpr (KIND == 0) {
        const size_t nblocks = (n + block - 1) / block;
        for (size_t blk = blockIdx.x; blk < nblocks && threadIdx.x < block; blk += gridDim.x) {
            const size_t i = blk * block + threadIdx.x;
            if (i >= n) break;
            uint32_t s[FRW];
            load_scalar(s, reinterpret_cast<const uint32_t*>(scalars), i, mont);
            uint32_t over = 0;
#pragma unroll
            for (int j = 0; j < FRW; ++j) {
                const int lo = limit_bits - 32 * j;   // bits of word j below the limit
                over |= lo <= 0 ? s[j] : (lo < 32 ? s[j] >> lo : 0u);
            }
            if (over) {
                atomicOr(flag, 1u);
#pragma unroll
                for (int j = 0; j < FRW; ++j) s[j] = 0;
            }
            for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
                digits[(size_t)w * stride + i] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(uint32_t)w * nbin + (idx >> fb)], 1u);
                }
            });
        }
    } else {
        constexpr int NW = KIND == 8 ? 2 : 1;
        const packed_split<KIND> sp(scalars, n);
        const size_t items = sp.items();
        auto recode = [&](uint64_t v, size_t i) {
            if (limit_bits < 8 * KIND && (v >> limit_bits) != 0) {
                atomicOr(flag, 1u);
                v = 0;
            }
            uint32_t s[NW];
            s[0] = (uint32_t)v;
            if (NW > 1) s[NW - 1] = (uint32_t)(v >> 32);
            for_each_signed_digit(s, c, W, [&](int w, int32_t d) {
                digits[(size_t)w * stride + i] = d;
                if (d != 0) {
                    const uint32_t idx = (uint32_t)(d < 0 ? -d : d) - 1u;
                    atomicAdd(&smem[(uint32_t)w * nbin + (idx >> fb)], 1u);
                }
            });
        };
        const size_t nblocks = (items + block - 1) / block;
        for (size_t blk = blockIdx.x; blk < nblocks && threadIdx.x < block; blk += gridDim.x) {
            const size_t t = blk * block + threadIdx.x;
            if (t >= items) break;
            if (t < sp.nvec) {
                uint32_t v[4];
                packed_vec(v, scalars, (sp.head * KIND) + t * 16);
                const size_t i0 = sp.head + t * packed_split<KIND>::EPL;
#pragma unroll
                for (int j = 0; j < packed_split<KIND>::EPL; ++j) recode(packed_elem<KIND>(v, j), i0 + j);
            } else {
                const size_t i = sp.single_index(t);
                recode(packed_one<KIND>(scalars, i), i);
            }
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nctr; j += SORT_TPB) {
        const uint32_t v = smem[j];
        if (v) atomicAdd(&coarse_counts[(j / nbin) * (nbin + 1) + (j % nbin)], v);
    }
}

// Workgroup (tile, w) of the coarse pass.  Two of them share a CU (profiles/r05_sort_two_workgroups.txt: one workgroup
// per CU spent three quarters of its wave-cycles waiting on the phase in front), so a tile costs 64 KiB of staging and
// at most 64 registers per lane:
//   * the staged key is the bucket index, 16 bits wide where c <= 17 (SK = unsigned short; 32 bits beyond, where the
//     96 KiB of staging leave one workgroup per CU as before),
//   * the staged payload is the entry's position inside the tile (14 bits) with the digit's sign in bit 15 -- the 32-bit
//     payload digit_payload(tile0 + position, d) is rebuilt at write-out (flat and split modes number their entries by
//     the column index too, so this holds for every mode),
//   * rank, sign and bucket index of an entry wait in ONE register for the run starts.
// The scan of the window's coarse counts is done here too, by every workgroup for itself in LDS (a launch of its own
// before): coarse[w][0..nbin) holds the COUNTS while this kernel runs, cursor[] starts at zero and hands out offsets
// inside a bin, and the workgroup that draws the last ticket of its window (coarse[w][nbin], zero on entry) replaces
// the counts by their exclusive starts and the ticket by the window total -- what k_sort_fine / k_sort_big_* read.
static_assert(SORT_TILE <= 16384 && SORT_TILE % SORT_TPB == 0, "a tile position is staged in 14 bits");
// the second argument of __launch_bounds__ counts waves per SIMD: two workgroups of SORT_TPB threads on the four SIMDs
// of a CU are 8, i.e. at most 64 registers per lane
constexpr int SORT_WAVES_2WG = 2 * SORT_TPB / 256;
constexpr uint32_t SORT_NONE = 0xffffffffu;
template <typename SK>
__global__ void __launch_bounds__(SORT_TPB, sizeof(SK) == 2 ? SORT_WAVES_2WG : SORT_TPB / 256)
    k_sort_coarse(const int32_t* __restrict__ digits, size_t n, size_t stride, int c, int hb, uint32_t* __restrict__ coarse,
                  uint32_t* __restrict__ cursor, uint32_t* __restrict__ tmp_payload, sort_key_t* __restrict__ tmp_key,
                  int dtop) {
    // tmp_key: the fine part of the bucket index (fb <= 11 bits) -- all the second level needs
    constexpr bool WIDE = sizeof(SK) != 2;
    __shared__ uint32_t hist[1 << SORT_MAX_HB], lstart[1 << SORT_MAX_HB], wbase[1 << SORT_MAX_HB], tmp[SORT_TPB / 64 + 1];
    __shared__ uint32_t last;
    __shared__ SK st_key[SORT_TILE];
    __shared__ unsigned short st_pos[SORT_TILE];
    uint32_t* gbase = hist;   // hist[j] is dead once slot j's global base has been reserved
    const uint32_t nbin = 1u << hb;
    const uint32_t w = blockIdx.y;
    const int fb = c - 1 - hb - (w == gridDim.y - 1u ? dtop : 0);   // the top window keeps fewer fine bits (sort_top_shift)
    const size_t tile0 = (size_t)blockIdx.x * SORT_TILE;
    uint32_t* cw = coarse + (size_t)w * (nbin + 1);
    for (uint32_t j = threadIdx.x; j < nbin; j += SORT_TPB) {
        hist[j] = 0;
        wbase[j] = cw[j];
    }
    __syncthreads();
    constexpr int PER = SORT_TILE / SORT_TPB;
    // ONE LDS atomic per entry: the histogram update returns the entry's rank inside its (tile, bin) run, kept in a
    // register until the run starts are known (a second, returning atomic on a cursor array used to hand the ranks out)
    // ent: rank (14 bits) | sign << 14 | bucket index << 15 (16-bit keys only), or SORT_NONE for a zero digit
    uint32_t ent[PER], idx[WIDE ? PER : 1];
    // (uniform base, 32-bit position: no 64-bit address per load in flight)
    const int32_t* dt = digits + ((size_t)w * stride + tile0);
    const uint32_t cnt = tile0 >= n ? 0u : (n - tile0 < (size_t)SORT_TILE ? (uint32_t)(n - tile0) : (uint32_t)SORT_TILE);
#pragma unroll
    for (int k = 0; k < PER; ++k) {   // all the loads first: the digit waits in the register its entry word takes
        const uint32_t loc = (uint32_t)k * SORT_TPB + threadIdx.x;
        ent[k] = (loc < cnt) ? (uint32_t)dt[loc] : 0u;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int32_t d = (int32_t)ent[k];
        const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u;
        const uint32_t r = d ? atomicAdd(&hist[b >> fb], 1u) : 0u;
        if constexpr (WIDE) {
            idx[k] = b;
            ent[k] = d ? (r | (d < 0 ? 0x4000u : 0u)) : SORT_NONE;
        } else {
            ent[k] = d ? (r | (d < 0 ? 0x4000u : 0u) | (b << 15)) : SORT_NONE;
        }
    }
    __syncthreads();
    const uint32_t total = block_exclusive_scan<SORT_TPB, (1 << SORT_MAX_HB) / SORT_TPB>(hist, lstart, nbin, tmp);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (ent[k] != SORT_NONE) {
            uint32_t b;
            if constexpr (WIDE)
                b = idx[k];
            else
                b = ent[k] >> 15;
            const uint32_t r = lstart[b >> fb] + (ent[k] & 0x3fffu);
            st_key[r] = (SK)b;
            st_pos[r] = (unsigned short)(((uint32_t)k * SORT_TPB + threadIdx.x) | ((ent[k] & 0x4000u) << 1));
        }
    }
    const uint32_t wtotal = block_exclusive_scan<SORT_TPB, (1 << SORT_MAX_HB) / SORT_TPB>(wbase, wbase, nbin, tmp);   // in place: it reads before it writes
    for (uint32_t j = threadIdx.x; j < nbin; j += SORT_TPB) {
        const uint32_t h = hist[j];
        gbase[j] = h ? wbase[j] + atomicAdd(&cursor[(size_t)w * nbin + j], h) : 0u;
    }
    // every thread's read of the counts lies before the first barrier, so the last ticket of a window is drawn after
    // the last read of its counts
    if (threadIdx.x == 0) last = atomicAdd(&cw[nbin], 1u) == gridDim.x - 1u;
    __syncthreads();
    if (last) {
        for (uint32_t j = threadIdx.x; j < nbin; j += SORT_TPB) cw[j] = wbase[j];
        if (threadIdx.x == 0) cw[nbin] = wtotal;
    }
    uint32_t* out_pay = tmp_payload + (size_t)w * stride;
    sort_key_t* out_key = tmp_key + (size_t)w * stride;
    for (uint32_t k = threadIdx.x; k < total; k += SORT_TPB) {
        const uint32_t key = st_key[k], p = st_pos[k];
        const uint32_t bin = key >> fb;
        const uint32_t pos = gbase[bin] + (k - lstart[bin]);
        out_pay[pos] = ((uint32_t)tile0 + (p & 0x3fffu)) | ((p & 0x8000u) << 16);   // = digit_payload(i, d)
        out_key[pos] = (sort_key_t)(key & ((1u << fb) - 1u));
    }
}

// NT threads per workgroup: 1024 for bins of tens of thousands of entries, 256 when a bin holds
// a few thousand at most (2^20-point inputs), where barriers between 16 waves would dominate.
// PER: entries per thread of a one-chunk bin, chunk_cap <= PER * NT.  The 1024-thread forms with PER < 16 (chunk_cap <=
// 12288: 72 KiB of staging at most) are built for two workgroups per CU (64 registers); with PER = 16 the staging leaves
// room for one.
template <int NT, int PER>
__global__ void __launch_bounds__(NT, NT == SORT_TPB ? (PER < 16 ? SORT_WAVES_2WG : SORT_TPB / 256) : 1) k_sort_fine(const uint32_t* __restrict__ tmp_payload,
                                                        const sort_key_t* __restrict__ tmp_key,
                                                        const uint32_t* __restrict__ coarse, size_t stride, int c, int hb,
                                                        uint32_t chunk_cap, uint32_t big_thresh, uint32_t big_cap,
                                                        uint32_t perchunk_words, uint32_t* __restrict__ big,
                                                        uint32_t* __restrict__ ends, uint32_t* __restrict__ lists, int dtop) {
    // dynamic LDS: 4 arrays of nfine words, chunk_cap payload words, chunk_cap fine keys (u16), perchunk_words words
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ uint32_t tmp[NT / 64 + 1];
    const uint32_t nbin = 1u << hb;
    const uint32_t bin = blockIdx.x, w = blockIdx.y;
    const bool top = dtop != 0 && w == gridDim.y - 1u;
    const int fb = c - 1 - hb - (top ? dtop : 0);   // the top window keeps fewer fine bits (sort_top_shift)
    const uint32_t nfine = 1u << fb, fmask = nfine - 1u;
    uint32_t* fstart = smem;
    uint32_t* chist = fstart + nfine;
    uint32_t* cstart = chist + nfine;
    uint32_t* ccur = cstart + nfine;
    uint32_t* st_payload = ccur + nfine;
    unsigned short* st_fine = reinterpret_cast<unsigned short*>(st_payload + chunk_cap);
    const uint32_t* cs = coarse + (size_t)w * (nbin + 1);
    // (the same in every lane: as scalars they make key / pay / out uniform bases, and a load costs one offset register)
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(cs[bin]), m = __builtin_amdgcn_readfirstlane(cs[bin + 1]) - b0;
    const sort_key_t* key = tmp_key + (size_t)w * stride + b0;
    const uint32_t* pay = tmp_payload + (size_t)w * stride + b0;
    uint32_t* out = lists + (size_t)w * stride + b0;
    uint32_t* e = ends + (((size_t)w << (c - 1)) + ((size_t)bin << fb));
    if (top) {
        // the 2^hb bins of the shifted window cover the first 2^(c - 1 - dtop) buckets; the rest is empty and its ends are
        // the window's total (k_accumulate reads the last one as the total, bucket_of_entry relies on the monotone tail):
        // every workgroup fills an equal share of them
        const uint32_t share = (1u << (fb + dtop)) - nfine, total = cs[nbin];
        uint32_t* tail = ends + (((size_t)w << (c - 1)) + ((size_t)nbin << fb) + (size_t)bin * share);
        for (uint32_t j = threadIdx.x; j < share; j += NT) tail[j] = total;
    }
    if (m > big_thresh) {
        // oversized bin (many equal or clustered scalars): leave it to the cooperative kernels
        // below; its bucket counts are gathered in ends[] first, so clear them
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) e[j] = 0;
        if (threadIdx.x == 0) {
            const uint32_t tiles = (m + SORT_TILE - 1) / SORT_TILE;
            const uint32_t slot = atomicAdd(&big[0], 1u);   // < big_cap: sum of m over such bins <= W * n
            uint32_t* rec = big + 4 + 4 * (size_t)slot;
            rec[0] = w;
            rec[1] = bin;
            rec[2] = atomicAdd(&big[1], tiles);
            rec[3] = tiles;
        }
        return;
    }
    // pass A: sizes of the fine buckets of this bin -> ends[]
    // A bin of several chunks keeps one histogram per chunk (perchunk: room for them behind the staging area), so that
    // pass B needs no second count of each chunk: two LDS atomics and two reads of the key per entry instead of three
    // (the fine pass is bound by them: 6.2 ms of a 2^26-point MSM).
    if (m <= chunk_cap) {
        // The bin is one chunk (every bin of a uniformly random input up to ~2^22 points): ONE LDS atomic per entry -- the
        // histogram update returns the entry's rank inside its bucket, kept in a register with the fine key (rank < chunk_cap
        // <= 2^14 | key << 14; PER per thread) until the
        // bucket starts are known -- one read of the key, and the staged chunk IS the bin's list.
        uint32_t fr[PER];
        if (m == 0) {
            for (uint32_t j = threadIdx.x; j < nfine; j += NT) e[j] = b0;
            return;
        }
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) chist[j] = 0;
        // all the loads first, unconditional (a position past the bin reads the bin's last entry and is dropped below) and
        // with no early exit from these loops: the arrays must stay registers
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint32_t k = threadIdx.x + (uint32_t)q * NT;
            fr[q] = (uint32_t)key[k < m ? k : m - 1u] & fmask;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint32_t k = threadIdx.x + (uint32_t)q * NT;
            const uint32_t r = k < m ? atomicAdd(&chist[fr[q]], 1u) : 0u;
            fr[q] = r | (fr[q] << 14);
        }
        __syncthreads();
        block_exclusive_scan<NT, (1 << SORT_MAX_FB) / NT>(chist, fstart, nfine, tmp);
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) e[j] = b0 + fstart[j] + chist[j];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint32_t k = threadIdx.x + (uint32_t)q * NT;
            if (k < m) st_payload[fstart[fr[q] >> 14] + (fr[q] & 0x3fffu)] = pay[k];
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < m; k += NT) out[k] = st_payload[k];
        return;
    }
    const uint32_t nch = (m + chunk_cap - 1) / chunk_cap;
    uint32_t* ch = reinterpret_cast<uint32_t*>(st_fine + chunk_cap);   // [nch][nfine]
    const bool split_hist = (size_t)nch * nfine <= perchunk_words;   // (nch >= 2: one-chunk bins took the path above)
    if (split_hist) {
        for (uint32_t j = threadIdx.x; j < nch * nfine; j += NT) ch[j] = 0;
        __syncthreads();
        for (uint32_t q = 0, c0 = 0; q < nch; ++q, c0 += chunk_cap) {   // chunk_cap: any multiple of NT
            const uint32_t cm = (m - c0 < chunk_cap) ? m - c0 : chunk_cap;
            for (uint32_t k = threadIdx.x; k < cm; k += NT) atomicAdd(&ch[q * nfine + (key[c0 + k] & fmask)], 1u);
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) {
            uint32_t t = 0;
            for (uint32_t q = 0; q < nch; ++q) t += ch[q * nfine + j];
            chist[j] = t;
        }
    } else {
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) chist[j] = 0;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < m; k += NT) atomicAdd(&chist[key[k] & fmask], 1u);
    }
    __syncthreads();
    block_exclusive_scan<NT>(chist, fstart, nfine, tmp);
    for (uint32_t j = threadIdx.x; j < nfine; j += NT) e[j] = b0 + fstart[j] + chist[j];
    __syncthreads();
    // pass B: chunk-wise counting sort; fstart[f] advances as chunks are placed
    uint32_t cidx = 0;
    for (uint32_t c0 = 0; c0 < m; c0 += chunk_cap, ++cidx) {
        const uint32_t cm = (m - c0 < chunk_cap) ? m - c0 : chunk_cap;
        const uint32_t* hist_c = split_hist ? ch + cidx * nfine : chist;   // this chunk's histogram
        if (!split_hist) {
            for (uint32_t j = threadIdx.x; j < nfine; j += NT) chist[j] = 0;
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < cm; k += NT) atomicAdd(&chist[key[c0 + k] & fmask], 1u);
            __syncthreads();
        }
        block_exclusive_scan<NT>(hist_c, cstart, nfine, tmp);
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) ccur[j] = cstart[j];
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < cm; k += NT) {
            const uint32_t f = key[c0 + k] & fmask;
            const uint32_t r = atomicAdd(&ccur[f], 1u);
            st_payload[r] = pay[c0 + k];
            st_fine[r] = (unsigned short)f;
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < cm; k += NT) {
            const uint32_t f = st_fine[k];
            out[fstart[f] + (k - cstart[f])] = st_payload[k];
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nfine; j += NT) fstart[j] += hist_c[j];
        __syncthreads();
    }
}

// Oversized coarse bins (k_sort_fine registered them in big[]: word 0 = bins, word 1 = tiles,
// then records {w, bin, first tile, tiles}, then one cursor row of 2^fb words per record).
// Tiles of SORT_TILE entries are spread over the whole grid: histogram by fine key with one
// global atomic per (tile, key), a scan per bin, then an LDS counting sort per tile that
// reserves its runs with one global atomic per (tile, key) -- the coarse pass again, one
// level down.  With no such bin all three kernels return at once.
struct big_tile {
    uint32_t rec, w, bin, k0, cm;   // record, window, coarse bin, first entry within the bin, entries
};
AMDMSM_DEV bool big_find_tile(const uint32_t* __restrict__ big, const uint32_t* __restrict__ coarse, uint32_t nbin,
                              uint32_t tile, uint32_t* sh, big_tile& bt, uint32_t& b0) {
    const uint32_t nbig = big[0];
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < nbig; r += SORT_TPB) {
        const uint32_t* rec = big + 4 + 4 * (size_t)r;
        if (tile >= rec[2] && tile < rec[2] + rec[3]) sh[0] = r;
    }
    __syncthreads();
    bt.rec = sh[0];
    const uint32_t* rec = big + 4 + 4 * (size_t)bt.rec;
    bt.w = rec[0];
    bt.bin = rec[1];
    const uint32_t* cs = coarse + (size_t)bt.w * (nbin + 1);
    b0 = cs[bt.bin];
    const uint32_t m = cs[bt.bin + 1] - b0;
    bt.k0 = (tile - rec[2]) * SORT_TILE;
    bt.cm = (m - bt.k0 < (uint32_t)SORT_TILE) ? m - bt.k0 : (uint32_t)SORT_TILE;
    return true;
}

__global__ void __launch_bounds__(SORT_TPB) k_sort_big_hist(const sort_key_t* __restrict__ tmp_key,
                                                            const uint32_t* __restrict__ coarse, size_t stride, int c,
                                                            int hb, const uint32_t* __restrict__ big,
                                                            uint32_t* __restrict__ ends, uint32_t wtop, int dtop) {
    __shared__ uint32_t hist[1 << SORT_MAX_FB], sh[1];
    const uint32_t nbin = 1u << hb;
    const uint32_t tiles = big[1];
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        big_tile bt;
        uint32_t b0;
        big_find_tile(big, coarse, nbin, tile, sh, bt, b0);
        const int fb = c - 1 - hb - (bt.w == wtop ? dtop : 0);   // fine bits of the bin's window (sort_top_shift)
        const uint32_t nfine = 1u << fb, fmask = nfine - 1u;
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB) hist[j] = 0;
        __syncthreads();
        const sort_key_t* key = tmp_key + (size_t)bt.w * stride + b0 + bt.k0;
        for (uint32_t k = threadIdx.x; k < bt.cm; k += SORT_TPB) atomicAdd(&hist[key[k] & fmask], 1u);
        __syncthreads();
        uint32_t* e = ends + (((size_t)bt.w << (c - 1)) + ((size_t)bt.bin << fb));
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB)
            if (hist[j]) atomicAdd(&e[j], hist[j]);
    }
}

__global__ void __launch_bounds__(SORT_TPB) k_sort_big_scan(const uint32_t* __restrict__ coarse, int c, int hb,
                                                            uint32_t big_cap, uint32_t* __restrict__ big,
                                                            uint32_t* __restrict__ ends, uint32_t wtop, int dtop) {
    __shared__ uint32_t cnt[1 << SORT_MAX_FB], out[1 << SORT_MAX_FB], tmp[SORT_TPB / 64 + 1];
    const uint32_t nbin = 1u << hb;
    const int fb_row = c - 1 - hb;   // a record's cursor row keeps its full length
    const uint32_t nbig = big[0];
    for (uint32_t r = blockIdx.x; r < nbig; r += gridDim.x) {
        const uint32_t* rec = big + 4 + 4 * (size_t)r;
        const uint32_t w = rec[0], bin = rec[1];
        const uint32_t b0 = coarse[(size_t)w * (nbin + 1) + bin];
        const int fb = fb_row - (w == wtop ? dtop : 0);
        const uint32_t nfine = 1u << fb;
        uint32_t* e = ends + (((size_t)w << (c - 1)) + ((size_t)bin << fb));
        uint32_t* cur = big + 4 + 4 * (size_t)big_cap + ((size_t)r << fb_row);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB) cnt[j] = e[j];
        __syncthreads();
        block_exclusive_scan(cnt, out, nfine, tmp);
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB) {
            cur[j] = b0 + out[j];
            e[j] = b0 + out[j] + cnt[j];
        }
    }
}

__global__ void __launch_bounds__(SORT_TPB, SORT_WAVES_2WG) k_sort_big_scatter(const uint32_t* __restrict__ tmp_payload,
                                                               const sort_key_t* __restrict__ tmp_key,
                                                               const uint32_t* __restrict__ coarse, size_t stride, int c,
                                                               int hb, uint32_t big_cap, uint32_t* __restrict__ big,
                                                               uint32_t* __restrict__ lists, uint32_t wtop, int dtop) {
    // dynamic LDS: hist / lstart / lcur / gbase of 2^fb words, then SORT_TILE source positions and SORT_TILE fine keys,
    // 16 bits each as in k_sort_coarse: the payload is fetched at write-out from the tile the position names
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ uint32_t tmp[SORT_TPB / 64 + 1], sh[1];
    const uint32_t nbin = 1u << hb;
    const int fb_row = c - 1 - hb;   // LDS layout and cursor rows keep the full length
    uint32_t* hist = smem;
    uint32_t* lstart = hist + (1u << fb_row);
    uint32_t* lcur = lstart + (1u << fb_row);
    uint32_t* gbase = lcur + (1u << fb_row);
    unsigned short* st_src = reinterpret_cast<unsigned short*>(gbase + (1u << fb_row));
    unsigned short* st_fine = st_src + SORT_TILE;
    const uint32_t tiles = big[1];
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        big_tile bt;
        uint32_t b0;
        big_find_tile(big, coarse, nbin, tile, sh, bt, b0);
        const int fb = fb_row - (bt.w == wtop ? dtop : 0);   // fine bits of the bin's window (sort_top_shift)
        const uint32_t nfine = 1u << fb, fmask = nfine - 1u;
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB) hist[j] = 0;
        __syncthreads();
        const sort_key_t* key = tmp_key + (size_t)bt.w * stride + b0 + bt.k0;
        const uint32_t* pay = tmp_payload + (size_t)bt.w * stride + b0 + bt.k0;
        for (uint32_t k = threadIdx.x; k < bt.cm; k += SORT_TPB) atomicAdd(&hist[key[k] & fmask], 1u);
        __syncthreads();
        block_exclusive_scan(hist, lstart, nfine, tmp);
        uint32_t* cur = big + 4 + 4 * (size_t)big_cap + ((size_t)bt.rec << fb_row);
        for (uint32_t j = threadIdx.x; j < nfine; j += SORT_TPB) {
            const uint32_t h = hist[j];
            lcur[j] = lstart[j];
            gbase[j] = h ? atomicAdd(&cur[j], h) : 0u;
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < bt.cm; k += SORT_TPB) {
            const uint32_t f = key[k] & fmask;
            const uint32_t r = atomicAdd(&lcur[f], 1u);
            st_src[r] = (unsigned short)k;
            st_fine[r] = (unsigned short)f;
        }
        __syncthreads();
        uint32_t* out = lists + (size_t)bt.w * stride;
        for (uint32_t k = threadIdx.x; k < bt.cm; k += SORT_TPB) {
            const uint32_t f = st_fine[k];
            out[gbase[f] + (k - lstart[f])] = pay[st_src[k]];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------ accumulation
// Work-balanced bucket accumulation.  Each lane owns S CONSECUTIVE entries of one window's
// bucket-sorted point list, whatever buckets they fall in (a segmented sum by key with
// fixed work per lane), so a wave's lanes finish together and a bucket of any size --
// e.g. the few, huge buckets of a short top window, or the "scalar == 1" bucket of a
// witness vector -- is simply spread over as many lanes as it needs.
//   * a bucket that lies entirely inside the lane's range is written straight to buckets[]
//   * the piece of a bucket that began in an earlier lane goes to part_first[lane]
//   * the piece of a bucket that continues into the next lane goes to part_last[lane]
//     and its bucket index to cont_bucket[lane]
// k_accumulate_fixup then closes every spanning bucket:
//   bucket = part_last[t] + part_first[t+1] + ... + part_first[lane of its last entry].
// buckets[] is zero-filled beforehand, so untouched (empty) buckets read as infinity.
// The accumulator of one lane of k_accumulate and what it does with it: XYZZ on almost-reduced 32-bit words
// (ec.cuh xyzz_madd_lz) or, for AMDMSM_ACC_RR groups, on reduced-radix limbs (rr.cuh xyzz_madd_rr: no carry
// instruction behind a multiply, limb-wise linear operations, an infinity flag instead of a zero test).
#if AMDMSM_ACC_RR
struct acc_state {
    XyzzRr<ERR> a;
    bool inf;
};
AMDMSM_DEV void acc_reset(acc_state& s) { s.inf = true; }   // the limbs are dead while inf is set
// the record as it is: this lane's 4 L limbs (all zero: infinity); its readers convert (load_xyzz_rec / rec_load_rho)
AMDMSM_DEV void acc_store(uint32_t* q, const acc_state& s) {
    uint4* q4 = reinterpret_cast<uint4*>(q + (GP::DEG == 2 && (threadIdx.x & 1u) ? 4 * RRL : 0));
    if (__builtin_expect(s.inf, 0)) {   // a bucket whose points cancelled (or a piece with infinite bases only)
#pragma unroll
        for (int i = 0; i < RRL; ++i) q4[i] = make_uint4(0, 0, 0, 0);
        return;
    }
    uint32_t w[4 * RRL];
#pragma unroll
    for (int i = 0; i < RRL; ++i) {
        w[i] = (uint32_t)re_limb(s.a.x, i);
        w[RRL + i] = (uint32_t)re_limb(s.a.y, i);
        w[2 * RRL + i] = (uint32_t)re_limb(s.a.zz, i);
        w[3 * RRL + i] = (uint32_t)re_limb(s.a.zzz, i);
    }
#pragma unroll
    for (int i = 0; i < RRL; ++i) q4[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
// this lane's component of one affine record (x, y) as words
struct aff_words {
    uint32_t x[FQ::N], y[FQ::N];
};
AMDMSM_DEV void aff_words_load(aff_words& p, const uint32_t* rec) {
    const uint4* r4 = reinterpret_cast<const uint4*>(rec + (GP::DEG == 2 && (threadIdx.x & 1u) ? FQ::N : 0));
#pragma unroll
    for (int i = 0; i < FQ::N / 4; ++i) {
        const uint4 a = r4[i], b = r4[EW / 4 + i];
        p.x[4 * i] = a.x; p.x[4 * i + 1] = a.y; p.x[4 * i + 2] = a.z; p.x[4 * i + 3] = a.w;
        p.y[4 * i] = b.x; p.y[4 * i + 1] = b.y; p.y[4 * i + 2] = b.z; p.y[4 * i + 3] = b.w;
    }
}
#else
struct acc_state {
    Xyzz<EA> a;
};
AMDMSM_DEV void acc_reset(acc_state& s) { xyzz_set_inf(s.a); }
AMDMSM_DEV void acc_store(uint32_t* q, acc_state& s) {
    xyzz_canon(s.a);
    store_xyzz(q, s.a);
}
AMDMSM_DEV void acc_add(acc_state& s, const uint32_t* rec, bool neg) {
    Aff<EA> p;
    load_aff(p, rec);
    el_cneg(p.y, p.y, neg);   // -(x, y) = (x, -y); (0,0) stays infinity
#if AMDMSM_ACC_LAZY
    xyzz_madd_lz(s.a, p);   // coordinates of acc stay in [0, 2p) between stores
#else
    xyzz_madd(s.a, p);
#endif
}
#endif

constexpr uint32_t NO_BUCKET = 0xffffffffu;

// A record of the bucket / partial arrays (ZZS words) comes in two forms:
//   * as k_accumulate wrote it (AMDMSM_ACC_RR): 4 L reduced-radix limbs per component, all zero = infinity;
//   * canonical (X, Y, ZZ, ZZZ) words at the start of the record (the 32-bit fallback of the fix-up kernels), with a mark
//     in the record's last word -- a word the canonical layout leaves free (ZZS > ZZW) and that in the limb form is the
//     top limb of ZZZ: a product's output or the constant one, far below 2^30 in magnitude, so that its bits 30 and 31
//     are equal there;
//   * a sum of the fix-up kernels on limbs (rec_sum_store): the limb layout with ALL FOUR coordinates carrying the factor
//     rho (k_accumulate's zz / zzz carry rho 2^D), marked by bit 31 of limb 0 of ZZ -- limbs 0 .. L-2 of ZZ are a
//     product's output in every state, in [0, 2^B).  Three quarters of the buckets of a 2^20-point MSM span two lanes
//     and are written this way: their readers need no conversion at all, and the writer no export.
// Every reader takes either (load_xyzz_rec): the limb form is turned into canonical words in registers -- one product by a
// power of two and one exact normalisation per coordinate (rr_export_component) -- which used to be a pass of its own over
// all records, read or not (k_rr_export: a memory round trip of 272 B per record, 3 % of a 2^20-point MSM).
#if AMDMSM_ACC_RR
static_assert(ZZS > ZZW, "a canonical record leaves the last word of the limb record free");
constexpr uint32_t REC_CANON_MARK = 0x40000000u;
template <class P, bool I> AMDMSM_DEV uint32_t (&lane_words(Fp<P, I>& a))[P::N] { return a.v; }
template <class P, int NR> AMDMSM_DEV uint32_t (&lane_words(Fp2H<P, NR>& a))[P::N] { return a.h.v; }
template <class T>
AMDMSM_DEV void load_xyzz_rec(Xyzz<T>& p, const uint32_t* q) {
    const uint32_t mk = q[ZZS - 1];
    if (((mk ^ (mk << 1)) >> 31) != 0) {   // canonical words
        load_xyzz(p, q);
        return;
    }
    // this lane's component: 4 L limbs (an Fq2 record: the even lane of the pair takes component 0, the odd lane 1)
    const uint4* q4 = reinterpret_cast<const uint4*>(q + (GP::DEG == 2 && (threadIdx.x & 1u) ? 4 * RRL : 0));
    uint32_t w[4 * RRL];
#pragma unroll
    for (int k = 0; k < RRL; ++k) {
        const uint4 v = q4[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    constexpr int D = rr_shape<FQ>::D;
    const bool rho = (w[2 * RRL] >> 31) != 0;   // a fix-up kernel's sum: zz, zzz with the factor rho
    w[2 * RRL] &= 0x7fffffffu;
    Rr<FQ> a;
    // (zero limbs give zero words: an all-zero record reads as ZZ == 0, infinity; a zero component of a finite Fq2
    // point stays zero)
#pragma unroll
    for (int k = 0; k < RRL; ++k) a.v[k] = (int32_t)w[k];
    rr_export_component<FQ, 0>(lane_words(p.x), a);
#pragma unroll
    for (int k = 0; k < RRL; ++k) a.v[k] = (int32_t)w[RRL + k];
    rr_export_component<FQ, 0>(lane_words(p.y), a);
#pragma unroll
    for (int k = 0; k < RRL; ++k) a.v[k] = (int32_t)w[2 * RRL + k];
    if (rho) rr_export_component<FQ, 0>(lane_words(p.zz), a);
    else rr_export_component<FQ, D>(lane_words(p.zz), a);
#pragma unroll
    for (int k = 0; k < RRL; ++k) a.v[k] = (int32_t)w[3 * RRL + k];
    if (rho) rr_export_component<FQ, 0>(lane_words(p.zzz), a);
    else rr_export_component<FQ, D>(lane_words(p.zzz), a);
}
template <class T>
AMDMSM_DEV void store_xyzz_rec(uint32_t* q, const Xyzz<T>& p) {
    store_xyzz(q, p);
    q[ZZS - 1] = REC_CANON_MARK;   // (both lanes of an Fq2 pair write the same word)
}
#else
template <class T> AMDMSM_DEV void load_xyzz_rec(Xyzz<T>& p, const uint32_t* q) { load_xyzz(p, q); }
template <class T> AMDMSM_DEV void store_xyzz_rec(uint32_t* q, const Xyzz<T>& p) { store_xyzz(q, p); }
#endif

// Running sum of records for the serial parts of the fix-up kernels and of k_bucket_sums: on reduced-radix limbs where
// k_accumulate writes them (rr.cuh xyzz_add_rho: every coordinate with the factor rho, 2 L^2 multiply issues per product,
// no carry instructions), on canonical words otherwise.  rec_sum_get hands the sum over as canonical words for the
// wave-level butterflies, which stay on fp.cuh's arithmetic.
#ifndef AMDMSM_SUM_RR
#define AMDMSM_SUM_RR AMDMSM_ACC_RR
#endif
#if AMDMSM_SUM_RR
struct rec_sum {
    XyzzRr<ERR> a;
    bool inf;
};
AMDMSM_DEV void rec_sum_init(rec_sum& s) {
    s.inf = true;
    re_zero(s.a.x); re_zero(s.a.y); re_zero(s.a.zz); re_zero(s.a.zzz);   // (the fold moves the limbs of infinite lanes too)
}
// the record at q on limbs, all four coordinates with the factor rho; inf: the record is the point at infinity
AMDMSM_DEV void rec_load_rho(XyzzRr<ERR>& p, bool& inf, const uint32_t* q) {
    const uint32_t mk = q[ZZS - 1];
    if (((mk ^ (mk << 1)) >> 31) != 0) {   // canonical words (a fix-up kernel's sum): one product per coordinate
        Xyzz<ER> c;
        load_xyzz(c, q);
        inf = xyzz_is_inf(c);
        re_from_words_rho(p.x, lane_words(c.x));
        re_from_words_rho(p.y, lane_words(c.y));
        re_from_words_rho(p.zz, lane_words(c.zz));
        re_from_words_rho(p.zzz, lane_words(c.zzz));
        return;
    }
    const uint4* q4 = reinterpret_cast<const uint4*>(q + (GP::DEG == 2 && (threadIdx.x & 1u) ? 4 * RRL : 0));
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < RRL; ++k) {
        const uint4 v = q4[k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * k + j;   // limb i % L of coordinate i / L
            int32_t& dst = i < RRL ? re_limb(p.x, i) : (i < 2 * RRL ? re_limb(p.y, i - RRL) : (i < 3 * RRL ? re_limb(p.zz, i - 2 * RRL) : re_limb(p.zzz, i - 3 * RRL)));
            dst = (int32_t)w[j];
            if (i >= 2 * RRL && i < 3 * RRL) any |= w[j];
        }
    }
    // k_accumulate writes infinity as an all-zero record; the zz of a finite point is never zero mod p, let alone on limbs
    inf = re_all<ERR>(any == 0);
    // a fix-up kernel's sum (rec_sum_store): every coordinate has the factor rho already
    const bool rho = re_limb(p.zz, 0) < 0;   // bit 31 of limb 0 of ZZ, which is never negative
    if (rho) re_limb(p.zz, 0) &= 0x7fffffff;
    else xyzz_rec_to_rho(p);
}
// the sum as a record of the third form (or an all-zero record: infinity)
AMDMSM_DEV void rec_sum_store(uint32_t* q, const rec_sum& s) {
    uint4* q4 = reinterpret_cast<uint4*>(q + (GP::DEG == 2 && (threadIdx.x & 1u) ? 4 * RRL : 0));
    uint32_t w[4 * RRL];
    const uint32_t keep = s.inf ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < RRL; ++i) {
        w[i] = (uint32_t)re_limb(s.a.x, i) & keep;
        w[RRL + i] = (uint32_t)re_limb(s.a.y, i) & keep;
        w[2 * RRL + i] = (uint32_t)re_limb(s.a.zz, i) & keep;
        w[3 * RRL + i] = (uint32_t)re_limb(s.a.zzz, i) & keep;
    }
    w[2 * RRL] |= 0x80000000u & keep;
#pragma unroll
    for (int i = 0; i < RRL; ++i) q4[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
AMDMSM_DEV void rec_sum_add(rec_sum& s, const uint32_t* q) {
    XyzzRr<ERR> b;
    bool b_inf;
    rec_load_rho(b, b_inf, q);
    xyzz_add_rho(s.a, s.inf, b, b_inf);
}
// the sums of G neighbouring reduction lanes (a reduction lane is RED_LANES physical lanes wide) folded into the first
// of them: XOR butterfly on limbs, infinity outside the data; every lane of the wave must call it
AMDMSM_DEV void rec_sum_fold(rec_sum& s, uint32_t G) {
    for (uint32_t off = 1; off < G; off <<= 1) {
        XyzzRr<ERR> o;
        const int m = (int)(off * RED_LANES);
#pragma unroll
        for (int i = 0; i < RRL; ++i) {
            re_limb(o.x, i) = __shfl_xor(re_limb(s.a.x, i), m, 64);
            re_limb(o.y, i) = __shfl_xor(re_limb(s.a.y, i), m, 64);
            re_limb(o.zz, i) = __shfl_xor(re_limb(s.a.zz, i), m, 64);
            re_limb(o.zzz, i) = __shfl_xor(re_limb(s.a.zzz, i), m, 64);
        }
        const bool o_inf = __shfl_xor(s.inf ? 1 : 0, m, 64) != 0;
        xyzz_add_rho(s.a, s.inf, o, o_inf);
    }
}
AMDMSM_DEV void rec_sum_get(Xyzz<ER>& out, const rec_sum& s) {
    if (s.inf) {
        xyzz_set_inf(out);
        return;
    }
    rr_export_component<FQ, 0>(lane_words(out.x), re_comp(s.a.x));
    rr_export_component<FQ, 0>(lane_words(out.y), re_comp(s.a.y));
    rr_export_component<FQ, 0>(lane_words(out.zz), re_comp(s.a.zz));
    rr_export_component<FQ, 0>(lane_words(out.zzz), re_comp(s.a.zzz));
}
#else
struct rec_sum {
    Xyzz<ER> a;
};
AMDMSM_DEV void rec_sum_init(rec_sum& s) { xyzz_set_inf(s.a); }
AMDMSM_DEV void rec_sum_add(rec_sum& s, const uint32_t* q) {
    Xyzz<ER> x;
    load_xyzz_rec(x, q);
    xyzz_add(s.a, s.a, x);
}
AMDMSM_DEV void rec_sum_get(Xyzz<ER>& out, const rec_sum& s) { out = s.a; }
AMDMSM_DEV void rec_sum_store(uint32_t* q, const rec_sum& s) { store_xyzz_rec(q, s.a); }
AMDMSM_DEV void wave_group_sum_r(Jac<ER>& p, uint32_t G);
AMDMSM_DEV void rec_sum_fold(rec_sum& s, uint32_t G) {
    Jac<ER> j;
    xyzz_to_jac(j, s.a);
    wave_group_sum_r(j, G);
    jac_to_xyzz(s.a, j);
}
#endif

// smallest b with e[b] > k   (e non-decreasing, e[B-1] > k)
AMDMSM_DEV uint32_t bucket_of_entry(const uint32_t* __restrict__ e, uint32_t B, uint32_t k) {
    uint32_t l = 0, r = B - 1;
    while (l < r) {
        const uint32_t m = (l + r) >> 1;
        if (e[m] > k) r = m; else l = m + 1;
    }
    return l;
}

__global__ void __launch_bounds__(TPB, AMDMSM_ACC_WAVES) k_accumulate(const uint32_t* __restrict__ ends, const uint32_t* __restrict__ lists,
                                                    size_t list_stride, const uint32_t* __restrict__ bases,
                                                    uint32_t* __restrict__ buckets, uint32_t* __restrict__ part_first,
                                                    uint32_t* __restrict__ part_last, uint32_t* __restrict__ cont_bucket,
                                                    int W, uint32_t B, uint32_t S, uint32_t T,
                                                    const uint32_t* __restrict__ endo_pts, uint32_t n_real, int sync_waves
#ifdef AMDMSM_ACC_TRACE
                                                    , unsigned long long* __restrict__ trace
#endif
                                                    ) {
#ifdef AMDMSM_ACC_TRACE
    // experiment: wall-clock (100 MHz) start / end of every wave, and where it ran
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    struct trace_end {
        unsigned long long* p;
        unsigned long long t0;
        __device__ ~trace_end() {
            if ((threadIdx.x & 63u) == 0) {
                const size_t wv = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
                p[3 * wv] = t0;
                p[3 * wv + 1] = __builtin_amdgcn_s_memrealtime();
                p[3 * wv + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((15 << 11) | 4) |
                                ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);   // HW_ID, XCC_ID
            }
        }
    } trace_guard{trace, t_start};
#endif
    // entries >= n_real (endomorphism split only; otherwise n_real = 2^31) name phi(P_(e - n_real)),
    // record e - n_real of endo_pts (k_endo_points)
    const size_t g = gtid() / ACC_LANES;   // split form: lanes 2g, 2g+1 work on the same entries
    const size_t w = g / T;
    const uint32_t t = (uint32_t)(g % T);
    if (w >= (size_t)W) return;
    const uint32_t* e = ends + w * B;
    const uint32_t total = e[B - 1];
    const uint32_t lo = t * S;
    if (lo >= total) {
        cont_bucket[g] = NO_BUCKET;
        return;
    }
    const uint32_t hi = (lo + S < total) ? lo + S : total;
    uint32_t b = bucket_of_entry(e, B, lo);
    uint32_t bend = e[b];
    // end of the bucket after the current one, fetched a whole bucket ahead: closing a bucket then
    // needs no load (a dependent global load there stalls the 64 lanes of the wave about once per
    // iteration when buckets hold ~S entries)
    uint32_t bnext = b + 1 < B ? e[b + 1] : 0xffffffffu;
    bool from_prev = (b ? e[b - 1] : 0u) < lo;   // first piece continues a bucket begun earlier
    const uint32_t* lst = lists + w * list_stride;
    uint32_t* bk = buckets + w * (size_t)B * ZZS;
    acc_state acc;
    acc_reset(acc);
    // The lane's list entries are staged through LDS sixteen at a time (sixteen loads issued
    // together, once per sixteen iterations): read one word per iteration, the 256 lanes of a
    // workgroup touch 256 different cache lines every iteration, the point gathers evict them in
    // between, and every line is fetched again for each of its entries (measured: half of the
    // kernel's memory traffic).  The last chunk of a lane may read up to 15 entries past its
    // range: the list allocation carries that much slack (make_plan).
    __shared__ uint32_t staged[16 * TPB];   // [entry in chunk][thread]: conflict-free both ways
    // The SIMD issues from its oldest ready wave first, so four equal waves that start together do
    // not finish together: traced at 2^20 points (tools/acc_trace.py) the four waves of a SIMD end
    // at 0.36 / 0.66 / 0.85 / 1.0 of the launch, and the last one runs alone -- at about 60 % of the
    // multiplier's rate -- for the final sixth.  Priorities that fall with progress (3 for the
    // first half of the lane's entries, 2 up to 7/8, 1 up to 15/16, then 0) let the waves that are
    // behind catch up at those marks, so that the four end within a few per cent of each other
    // (what is left is the spread between XCDs): 1.58 -> 1.41 ms in the traced build.
#ifndef AMDMSM_ACC_PRIO
#define AMDMSM_ACC_PRIO 1
#endif
#if AMDMSM_ACC_PRIO
    // (only for launches of one or two rounds of resident waves -- sync_waves: in a long launch the
    // newcomers' high priority holds back the waves that are about to free their slots, 2^24 points:
    // 18.0 -> 18.8 ms, 2^26: 67.3 -> 68.8)
    // (sync_waves == 2, overlap mode: one level down -- 2, 1, 0 -- so that the tail kernels of the MSM in front,
    // which run at priority 3, win the SIMD whenever they have an instruction ready)
    const uint32_t span_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)S);
    const uint32_t mark1 = sync_waves ? span_u / 2 : 0xffffffffu, mark2 = sync_waves ? span_u - span_u / 8 : 0xffffffffu,
                   mark3 = sync_waves ? span_u - span_u / 16 : 0xffffffffu;
    if (sync_waves == 1) __builtin_amdgcn_s_setprio(3);
    if (sync_waves == 2) __builtin_amdgcn_s_setprio(2);
#endif
#if AMDMSM_ACC_RR
    // The point of iteration k + 1 is fetched in the middle of iteration k (xyzz_madd_rr's mid hook): its words
    // take the registers the limbs of point k leave, and the gather's latency lies under eight products instead
    // of in front of the first one (three waves per SIMD do not cover it as four did for the 32-bit loop).
    aff_words pw;
    bool pneg = false;
    auto stage = [&](uint32_t k0) {   // list entries k0 .. k0 + 15 of this lane into its LDS column
        uint32_t v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = lst[k0 + q];
#pragma unroll
        for (int q = 0; q < 16; ++q) staged[q * TPB + threadIdx.x] = v[q];
    };
    auto fetch = [&](uint32_t k1) {
        const uint32_t ent = staged[((k1 - lo) & 15u) * TPB + threadIdx.x];
        const uint32_t pi = ent & 0x7fffffffu;
        aff_words_load(pw, pi >= n_real ? endo_pts + (size_t)(pi - n_real) * AFFW : bases + (size_t)pi * AFFW);
        pneg = (ent >> 31) != 0;
    };
    stage(lo);
    fetch(lo);
    for (uint32_t k = lo; k < hi; ++k) {
#if AMDMSM_ACC_PRIO
        {
            const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k - lo));
            if (sync_waves == 1) {
                if (j == mark1) __builtin_amdgcn_s_setprio(2);
                if (j == mark2) __builtin_amdgcn_s_setprio(1);
                if (j == mark3) __builtin_amdgcn_s_setprio(0);
            } else {
                if (j == mark1) __builtin_amdgcn_s_setprio(1);
                if (j == mark2) __builtin_amdgcn_s_setprio(0);
            }
        }
#endif
        if (k == bend) {
            // bucket b ends here: it is complete unless its head lies in an earlier lane
            // (round 4 measured two cheaper forms of this block -- the limbs stored straight from the accumulator registers
            // with the all-zero record out of line, 160 instead of 230 instructions, and the next end requested before the
            // stores -- and found no difference on one box, profiles/r04_experiments.txt: the block is not what a boundary costs)
            acc_store(from_prev ? part_first + g * ZZS : bk + (size_t)b * ZZS, acc);
            from_prev = false;
            acc_reset(acc);
            do {
                ++b;
                bend = bnext;
                bnext = b + 1 < B ? e[b + 1] : 0xffffffffu;
            } while (bend == k);   // skip empty buckets (k < total = e[B-1] bounds the walk)
        }
        const bool neg = pneg;
        xyzz_madd_rr(acc.a, acc.inf, pw.x, pw.y, neg, [&] {
            if (k + 1 < hi) {
                if (((k + 1 - lo) & 15u) == 0) stage(k + 1);
                fetch(k + 1);
            }
        });
    }
#else
    for (uint32_t k = lo; k < hi; ++k) {
#if AMDMSM_ACC_PRIO
        {
            const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k - lo));
            if (sync_waves == 1) {
                if (j == mark1) __builtin_amdgcn_s_setprio(2);
                if (j == mark2) __builtin_amdgcn_s_setprio(1);
                if (j == mark3) __builtin_amdgcn_s_setprio(0);
            } else {
                if (j == mark1) __builtin_amdgcn_s_setprio(1);
                if (j == mark2) __builtin_amdgcn_s_setprio(0);
            }
        }
#endif
        const uint32_t kk = (k - lo) & 15u;
        if (kk == 0) {
            uint32_t v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = lst[k + q];
#pragma unroll
            for (int q = 0; q < 16; ++q) staged[q * TPB + threadIdx.x] = v[q];
        }
        if (k == bend) {
            // bucket b ends here: it is complete unless its head lies in an earlier lane
            acc_store(from_prev ? part_first + g * ZZS : bk + (size_t)b * ZZS, acc);
            from_prev = false;
            acc_reset(acc);
            do {
                ++b;
                bend = bnext;
                bnext = b + 1 < B ? e[b + 1] : 0xffffffffu;
            } while (bend == k);   // skip empty buckets (k < total = e[B-1] bounds the walk)
        }
        const uint32_t ent = staged[kk * TPB + threadIdx.x];
#ifdef AMDMSM_EXP_BASE_MASK
        // timing experiment only (wrong results): every base read lands in the first 2^MASK records, i.e. in the
        // Infinity Cache -- the upper bound of what processing the input in cache-sized slices could save here
        const uint32_t pi = ent & ((1u << AMDMSM_EXP_BASE_MASK) - 1u);
#else
        const uint32_t pi = ent & 0x7fffffffu;
#endif
        acc_add(acc, pi >= n_real ? endo_pts + (size_t)(pi - n_real) * AFFW : bases + (size_t)pi * AFFW, (ent >> 31) != 0);
    }
#endif
    if (bend == hi) {   // the last bucket ends exactly with the lane
        acc_store(from_prev ? part_first + g * ZZS : bk + (size_t)b * ZZS, acc);
        cont_bucket[g] = NO_BUCKET;
    } else if (from_prev) {   // the whole lane lies inside one bucket
        acc_store(part_first + g * ZZS, acc);
        cont_bucket[g] = NO_BUCKET;
    } else {   // bucket b starts in this lane and continues
        acc_store(part_last + g * ZZS, acc);
        cont_bucket[g] = b;
    }
}

AMDMSM_DEV void wave_group_sum(Jac<E>& p, uint32_t G);
AMDMSM_DEV void wave_group_sum_r(Jac<ER>& p, uint32_t G);

// Closing the spanning buckets.  A span of up to INLINE_SPAN further lanes is summed by the
// lane's own thread (the common case: buckets of about S entries); longer ones are queued and
// closed by MID_G lanes each (up to MID_SPAN lanes: buckets of a few thousand entries, the
// regime of a precomputed-table MSM or a short top window) or by a whole wave (a bucket holding
// a large share of the input), so that no wave idles behind a single long serial sum.
// (8-limb fields: 3 -- the short top window of the endomorphism split, ~2.3 S entries per bucket,
// then stays out of the queue: reduction phase 0.66 -> 0.63 ms at 2^20, 0.61 -> 0.57 at 2^16,
// alt_bn128 G2 1.27 -> 1.11; the longer additions of 12- and 24-limb fields make the third serial
// addition cost more than the queue pass: bls12_377 G2 2.92 -> 3.31 ms, so 2 there)
#ifdef AMDMSM_INLINE_SPAN
constexpr uint32_t INLINE_SPAN = AMDMSM_INLINE_SPAN;
#else
constexpr uint32_t INLINE_SPAN = FQ::N <= 8 ? 3 : 2;
#endif
constexpr uint32_t MID_SPAN = 32;
constexpr uint32_t MID_G = 8;

// queue layout (fixup_queue_words): [0] long count, [1] mid count, long entries, mid entries
AMDMSM_DEV uint32_t* fixup_queue_base(uint32_t* q, size_t lanes, int mid) {
    return q + 2 + (mid ? 2 * fixup_queue_cap_long(lanes) : 0);
}

// (The fix-up kernels hold their elements as the bucket reduction does -- ER: an Fq2 element over a pair of lanes for the
// groups built with AMDMSM_ACC_SPLIT, RED_LANES physical lanes per logical lane -- so that they are not the one-wave-per-SIMD
// kernels with spill space the packed form made them: bls12_377 G2 2^21 fix-up 1.16 -> see profiles/r03_experiments.txt.)
AMDMSM_DEV void fixup_compact_block(uint32_t blk, const uint32_t* __restrict__ ends, uint32_t* __restrict__ part_first, int W,
                                    uint32_t B, uint32_t S, uint32_t T);

// blocks [0, fix_blocks): the spans; blocks from fix_blocks on: the folding of aligned blocks inside very long spans
// (fixup_compact_block below) -- independent work in one launch: an inline span never reaches a folded block's first
// slot, which only the queue pass that follows reads
__global__ void __launch_bounds__(64, AMDMSM_TAIL_WAVES) k_accumulate_fixup(const uint32_t* __restrict__ ends,
                                                         uint32_t* __restrict__ part_first,
                                                         const uint32_t* __restrict__ part_last,
                                                         const uint32_t* __restrict__ cont_bucket,
                                                         uint32_t* __restrict__ buckets, uint32_t* __restrict__ queue,
                                                         int W, uint32_t B, uint32_t S, uint32_t T, uint32_t fix_blocks) {
    if (blockIdx.x >= fix_blocks) {
        fixup_compact_block(blockIdx.x - fix_blocks, ends, part_first, W, B, S, T);
        return;
    }
    const size_t g = gtid() / RED_LANES;
    const bool first_of_pair = (threadIdx.x % RED_LANES) == 0;
    const size_t w = g / T;
    const uint32_t t = (uint32_t)(g % T);
    uint32_t b = NO_BUCKET, t_last = 0;
    if (w < (size_t)W) {
        b = cont_bucket[g];
        if (b != NO_BUCKET) t_last = (ends[w * B + b] - 1) / S;   // lane holding the bucket's last entry
    }
    const uint32_t span = (b != NO_BUCKET) ? t_last - t : 0;
    // queue the longer spans, one atomic per wave and class
    const size_t lanes = (size_t)W * T;
#pragma unroll
    for (int mid = 0; mid < 2; ++mid) {
        const bool mine = first_of_pair && (mid ? (span > INLINE_SPAN && span <= MID_SPAN) : (span > MID_SPAN));
        const unsigned long long m = __ballot(mine);
        if (m == 0) continue;
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t base = 0;
        if (lane == (uint32_t)__ffsll((long long)m) - 1u) base = atomicAdd(&queue[mid], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, __ffsll((long long)m) - 1, 64);
        if (mine) {
            const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            uint32_t* q = fixup_queue_base(queue, lanes, mid);
            q[2 * (size_t)slot] = (uint32_t)g;
            q[2 * (size_t)slot + 1] = (uint32_t)(g >> 32);
        }
    }
    if (span == 0 || span > INLINE_SPAN) return;
    rec_sum sum;
    rec_sum_init(sum);
    rec_sum_add(sum, part_last + g * ZZS);
#ifndef AMDMSM_FIX_PRIO
#define AMDMSM_FIX_PRIO 1
#endif
    // priority falling with progress, as in k_accumulate: the waves of a SIMD end together
    if (AMDMSM_FIX_PRIO) __builtin_amdgcn_s_setprio(3);
    for (uint32_t u = t + 1; u <= t_last; ++u) {
        rec_sum_add(sum, part_first + (w * T + u) * ZZS);
        if (AMDMSM_FIX_PRIO) {
            const uint32_t done = (uint32_t)__builtin_amdgcn_readfirstlane((int)(u - t));
            if (done == 1) __builtin_amdgcn_s_setprio(2);
            if (done == 2) __builtin_amdgcn_s_setprio(1);
            if (done >= 3) __builtin_amdgcn_s_setprio(0);
        }
    }
    rec_sum_store(buckets + (w * B + b) * ZZS, sum);
}

// A bucket that spans thousands of lanes (one scalar value repeated across much of the input)
// would leave its queue entry's wave with a long serial sum.  Beforehand, every aligned block
// of FIX_BLOCK lanes that lies wholly inside one such span is folded by a wave of its own into
// the block's first part_first slot; the closing wave then reads one partial per block.
constexpr uint32_t FIX_BLOCK = 256;

AMDMSM_DEV void fixup_compact_block(uint32_t blk, const uint32_t* __restrict__ ends, uint32_t* __restrict__ part_first, int W,
                                    uint32_t B, uint32_t S, uint32_t T) {
    const uint32_t nblk = T / FIX_BLOCK;
    if (nblk < 2) return;
    const size_t w = blk / (nblk - 1);
    const uint32_t k = blk % (nblk - 1) + 1;   // block 0 has no lane before it
    if (w >= (size_t)W) return;
    const uint32_t* e = ends + w * B;
    const uint32_t total = e[B - 1];
    const uint32_t first = k * FIX_BLOCK, last = first + FIX_BLOCK - 1;
    const uint64_t ent_a = (uint64_t)first * S - 1, ent_b = (uint64_t)last * S;
    if (ent_b >= total) return;
    // the bucket of the last entry before the block still runs in the block's last lane
    if (bucket_of_entry(e, B, (uint32_t)ent_a) != bucket_of_entry(e, B, (uint32_t)ent_b)) return;
    const uint32_t lane = (threadIdx.x & 63u) / RED_LANES;   // reduction lane of the wave, RED_FOLD of them
    rec_sum sum;
    rec_sum_init(sum);
    for (uint32_t u = first + lane; u <= last; u += RED_FOLD) rec_sum_add(sum, part_first + (w * T + u) * ZZS);
    rec_sum_fold(sum, RED_FOLD);
    if (lane == 0) rec_sum_store(part_first + (w * T + first) * ZZS, sum);
}

// G lanes per queued bucket (G = 64 for the long queue, MID_G for the mid queue): the lanes
// stride over its partials (one per folded block, see k_accumulate_compact), XOR butterfly,
// the group's first lane stores
__global__ void __launch_bounds__(64, AMDMSM_TAIL_WAVES) k_accumulate_fixup_queue(const uint32_t* __restrict__ ends,
                                                               const uint32_t* __restrict__ part_first,
                                                               const uint32_t* __restrict__ part_last,
                                                               const uint32_t* __restrict__ cont_bucket,
                                                               uint32_t* __restrict__ buckets,
                                                               const uint32_t* __restrict__ queue, uint32_t mid_blocks,
                                                               size_t lanes, uint32_t B, uint32_t S, uint32_t T) {
    // blocks [0, mid_blocks): the mid queue (MID_G lanes per bucket); the others: the long queue (a wave per bucket)
    __builtin_amdgcn_s_setprio(3);
    const int mid = blockIdx.x < mid_blocks ? 1 : 0;
    uint32_t G = mid ? MID_G : 64u;
    const uint32_t bid = mid ? blockIdx.x : blockIdx.x - mid_blocks, nblk = mid ? mid_blocks : gridDim.x - mid_blocks;
    const uint32_t count = queue[mid];
    const uint32_t* qb = queue + 2 + (mid ? 2 * fixup_queue_cap_long(lanes) : 0);
    if (G > RED_FOLD) G = RED_FOLD;   // a wave holds RED_FOLD reduction lanes
    // every field product costs a wave about a microsecond whatever its lane count, so with
    // many queued buckets fewer lanes each (about one wave per SIMD in total) finish sooner -- in both queues: the
    // short top window of a large MSM queues thousands of buckets of ~64 lanes each (2^26 points, c = 20: 8192 of them;
    // a wave per bucket took 0.85 ms, eight lanes per bucket take 0.2)
    while (G > 1 && (size_t)count * G * RED_LANES > 65536) G >>= 1;
    const uint32_t per_wave = RED_FOLD / G;
    const uint32_t rl = (threadIdx.x & 63u) / RED_LANES;   // reduction lane inside the wave
    const uint32_t sub = rl / G, lane = rl % G;
    for (uint32_t q0 = bid * per_wave; q0 < count; q0 += nblk * per_wave) {
        const uint32_t q = q0 + sub;
        const bool live = q < count;
        rec_sum sum;
        rec_sum_init(sum);
        size_t w = 0;
        uint32_t b = 0;
        if (live) {
            const size_t g = (size_t)qb[2 * (size_t)q] | ((size_t)qb[2 * (size_t)q + 1] << 32);
            w = g / T;
            const uint32_t t = (uint32_t)(g % T);
            b = cont_bucket[g];
            const uint32_t t_last = (ends[w * B + b] - 1) / S;
            if (lane == 0) rec_sum_add(sum, part_last + g * ZZS);
            // lanes t+1 .. t_last = head [t+1, h), nb folded blocks from h, tail [tail0, t_last]
            uint32_t h = (t + 1 + FIX_BLOCK - 1) / FIX_BLOCK * FIX_BLOCK;
            uint32_t nb = 0;
            if (h <= t_last + 1) nb = (t_last + 1 - h) / FIX_BLOCK; else h = t_last + 1;
            const uint32_t nh = h - (t + 1), tail0 = h + nb * FIX_BLOCK;
            const uint32_t items = nh + nb + (t_last + 1 - tail0);
            for (uint32_t i = lane; i < items; i += G) {
                const uint32_t u = i < nh ? t + 1 + i : (i < nh + nb ? h + (i - nh) * FIX_BLOCK : tail0 + (i - nh - nb));
                rec_sum_add(sum, part_first + (w * T + u) * ZZS);
            }
        }
        rec_sum_fold(sum, G);
        if (live && lane == 0) rec_sum_store(buckets + (w * B + b) * ZZS, sum);
    }
}

// --------------------------------------------------------------- reduction
// Wave-level plain sum: lanes whose index differs only in the low log2(G) bits are summed
// into the lane with those bits clear (XOR butterfly over ds_bpermute).  Every lane of the
// wave must call it; lanes outside the data carry infinity.
AMDMSM_DEV void wave_group_sum(Jac<E>& p, uint32_t G) {
    Jac<E> other;
    for (uint32_t off = 1; off < G; off <<= 1) {
        jac_shfl_xor(other, p, (int)off);
        jac_add(p, p, other);
    }
}

// Wave-level plain sum over RED_FOLD neighbouring reduction lanes (a reduction lane is RED_LANES
// physical lanes wide): XOR butterfly, infinity outside the data.
AMDMSM_DEV void wave_group_sum_r(Jac<ER>& p, uint32_t G) {
    Jac<ER> other;
    for (uint32_t off = 1; off < G; off <<= 1) {
        jac_shfl_xor(other, p, (int)(off * RED_LANES));
        jac_add(p, p, other);
    }
}

// sum_b (b + 1) * B_b for one window, first level: each lane takes L consecutive buckets
// with the running-sum recurrence of multiexp_accumulate_buckets (multiexp.tcc:109-122),
// adds (s*L) * (plain sum) for the weight offset of its segment, and the wave then folds
// G = min(M, RED_FOLD) neighbouring segments.  out[w][s / G].
__global__ void __launch_bounds__(64) k_reduce_segments(const uint32_t* __restrict__ buckets, int W, uint32_t B,
                                                        uint32_t L, uint32_t* __restrict__ out) {
    const size_t t = gtid() / RED_LANES;
    const uint32_t M = B / L;
    const uint32_t G = M < RED_FOLD ? M : RED_FOLD;
    const size_t w = t / M;
    const uint32_t s = (uint32_t)(t % M);
    const bool valid = w < (size_t)W;
    Jac<ER> acc, sum, bk;
    jac_set_inf(acc);
    jac_set_inf(sum);
    if (valid) {
        const uint32_t* seg = buckets + (w * B + (size_t)s * L) * ZZS;
        Xyzz<ER> xa, xs, xb;
        xyzz_set_inf(xa);
        xyzz_set_inf(xs);
        for (uint32_t j = L; j-- > 0;) {
            load_xyzz_rec(xb, seg + (size_t)j * ZZS);
            xyzz_add(xa, xa, xb);    // xa = sum_{k >= j} B_k
            xyzz_add(xs, xs, xa);    // xs = sum_k (k - j + 1) B_k
        }
        xyzz_to_jac(acc, xa);
        xyzz_to_jac(sum, xs);
        // segment's buckets carry weights s*L + j + 1: add (s*L) * acc
        jac_mul_u64(bk, acc, (unsigned long long)s * L);
        jac_add(sum, sum, bk);
    }
    wave_group_sum_r(sum, G);
    if (valid && (s % G) == 0) store_jac(out + (w * (M / G) + s / G) * XYZW, sum);
}

// plain sums: out[w][i / G] = sum of in[w][i .. i + G), G = min(M, RED_FOLD)
__global__ void __launch_bounds__(64) k_sum_butterfly(const uint32_t* __restrict__ in, int W, uint32_t M,
                                                      uint32_t* __restrict__ out) {
    const size_t t = gtid() / RED_LANES;
    const uint32_t G = M < RED_FOLD ? M : RED_FOLD;
    const size_t w = t / M;
    const uint32_t i = (uint32_t)(t % M);
    const bool valid = w < (size_t)W;
    Jac<ER> p;
    if (valid) load_jac(p, in + t * XYZW); else jac_set_inf(p);
    wave_group_sum_r(p, G);
    if (valid && (i % G) == 0) store_jac(out + (w * (M / G) + i / G) * XYZW, p);
}

// The last levels of the plain sums in one launch: one workgroup per window folds its M <=
// 256 / RED_LANES points -- every wave its RED_FOLD, then the first wave the per-wave results
// (through LDS) -- instead of a launch (and a lone-wave addition chain) per level.  out[w].
__global__ void __launch_bounds__(256) k_sum_block(const uint32_t* __restrict__ in, int W, uint32_t M,
                                                    uint32_t* __restrict__ out) {
    __shared__ uint32_t part[4 * XYZW];
    const size_t w = blockIdx.x;
    const uint32_t i = threadIdx.x / RED_LANES;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    Jac<ER> p;
    if (i < M) load_jac(p, in + (w * M + i) * XYZW); else jac_set_inf(p);
    wave_group_sum_r(p, RED_FOLD);
    if (lane < (uint32_t)RED_LANES) store_jac(part + wave * XYZW, p);
    __syncthreads();
    if (wave != 0) return;
    const uint32_t j = lane / RED_LANES;
    if (j < nw) load_jac(p, part + j * XYZW); else jac_set_inf(p);
    uint32_t G = 1;
    while (G < nw) G <<= 1;
    wave_group_sum_r(p, G);
    if (lane < (uint32_t)RED_LANES) store_jac(out + w * XYZW, p);
}

// The same with the last levels on lane-split elements: a per-lane addition costs a lone wave its
// whole latency however few lanes are live (~14 us for 8 words, ~40 us for Fq2 over 12, ~125 us for
// 24 words), a lane-split addition a quarter to a sixth of that, so once few points per window
// remain it is faster to give every wave one addition at a time.  Every wave first folds groups
// of 4 per-lane (two levels), the partial sums go to LDS, and the waves of the workgroup then
// halve them round by round (ping-pong LDS buffers).  out[w].
constexpr int SUMW_THREADS = (GP::DEG == 1 && FQ::N < 16) ? 512 : 256;
constexpr int SUMW_SLOTS = SUMW_THREADS / RED_LANES / 4;
template <class Q = FQ>
AMDMSM_DEV void sum_wide_add(const WideEnv<Q>& env, const uint32_t* a, const uint32_t* b, uint32_t* o) {
    if constexpr (GP::DEG == 2) {
        using F = WideFq2<Q, (GP::NR_SMALL == 0 ? -1 : GP::NR_SMALL)>;
        const uint32_t wi = F::word_index(env);
        uint32_t X1 = env.valid ? a[wi] : 0u, Y1 = env.valid ? a[EW + wi] : 0u, Z1 = env.valid ? a[2 * EW + wi] : 0u;
        const uint32_t X2 = env.valid ? b[wi] : 0u, Y2 = env.valid ? b[EW + wi] : 0u, Z2 = env.valid ? b[2 * EW + wi] : 0u;
        jac_add_seq<F, Q, GP::COEFF_A>(env, X1, Y1, Z1, X2, Y2, Z2);
        if (((threadIdx.x & 63u) >> 4) < 2 && env.valid) {
            o[wi] = X1;
            o[EW + wi] = Y1;
            o[2 * EW + wi] = Z1;
        }
    } else {
        uint32_t X1 = env.valid ? a[env.j] : 0u, Y1 = env.valid ? a[EW + env.j] : 0u, Z1 = env.valid ? a[2 * EW + env.j] : 0u;
        const uint32_t X2 = env.valid ? b[env.j] : 0u, Y2 = env.valid ? b[EW + env.j] : 0u, Z2 = env.valid ? b[2 * EW + env.j] : 0u;
        if constexpr (Q::N < 16) jac_add_wide<Q, GP::COEFF_A>(env, X1, Y1, Z1, X2, Y2, Z2);
        else jac_add_seq<WideFq<Q>, Q>(env, X1, Y1, Z1, X2, Y2, Z2);
        if ((threadIdx.x & 63u) < (uint32_t)Q::N) {
            o[env.j] = X1;
            o[EW + env.j] = Y1;
            o[2 * EW + env.j] = Z1;
        }
    }
}
__global__ void __launch_bounds__(SUMW_THREADS) k_sum_block_wide(const uint32_t* __restrict__ in, int W, uint32_t M,
                                                                 uint32_t* __restrict__ out) {
    __shared__ uint32_t buf[2][SUMW_SLOTS * XYZW];
    __builtin_amdgcn_s_setprio(3);
    const size_t w = blockIdx.x;
    const uint32_t i = threadIdx.x / RED_LANES, wave = threadIdx.x >> 6;   // i: reduction lane
    constexpr uint32_t NWAVES = SUMW_THREADS / 64;
    Jac<ER> p;
    if (i < M) load_jac(p, in + (w * M + i) * XYZW); else jac_set_inf(p);
    wave_group_sum_r(p, 4);
    if ((i & 3u) == 0) store_jac(buf[0] + (size_t)(i >> 2) * XYZW, p);
    __syncthreads();
    const WideEnv<FQ> env = wide_env<FQ>();
    uint32_t K = (M + 3) / 4;   // partial sums (M is a power of two >= 8)
    int cur = 0;
    while (K > 1) {
        const uint32_t pairs = K / 2;
        for (uint32_t q = wave; q < pairs; q += NWAVES) {   // wave-uniform
            const uint32_t* a = buf[cur] + (size_t)(2 * q) * XYZW;
            sum_wide_add(env, a, a + XYZW, buf[cur ^ 1] + (size_t)q * XYZW);
        }
        __syncthreads();
        cur ^= 1;
        K = pairs;
    }
    for (uint32_t t = threadIdx.x; t < (uint32_t)XYZW; t += SUMW_THREADS) out[w * XYZW + t] = buf[cur][t];
}

// ---- bucket reduction without per-segment multiples (the default from AMDMSM_ROWCOL_MIN_C up) ----
// sum_b (b + 1) B_b (multiexp_accumulate_buckets, multiexp.tcc:90-125) = sum_k 2^k P_k with the bit planes
// P_k = sum of the buckets whose weight b + 1 has bit k set.  The weights 1 .. B (B = 2^(c-1)) are laid
// out as a matrix, b + 1 = hi * C + lo with C = 2^h columns (h = ceil((c-1)/2)) and rows hi = 0 .. R
// (R = B / C; row R holds the single weight B):
//   k_bucket_sums    row[hi] = sum_lo bucket(hi, lo) and col[lo] = sum_hi bucket(hi, lo): two plain
//                    additions per bucket, q in the lane and a butterfly over the len / q lanes of a sum
//   k_plane_sums     P_k from the C column sums (k < h: columns whose index has bit k) or the R + 1 row
//                    sums (k >= h): one workgroup per (window, plane), at most max(C, R) / 2 inputs
//   k_window_horner  sum_k 2^k P_k per window, one wave each on lane-split elements (horner_chain with
//                    one doubling between planes)
// Against k_reduce_segments this removes the (segment offset) x (segment sum) multiples -- 13 doublings
// and up to 13 additions per lane at 2^20 points, two thirds of that kernel's field products -- and every
// level is a plain sum.
__global__ void __launch_bounds__(64, AMDMSM_TAIL_WAVES) k_bucket_sums(const uint32_t* __restrict__ buckets, int W, uint32_t B, int h,
                                                    uint32_t q_row, uint32_t q_col, uint32_t row_blocks,
                                                    uint32_t* __restrict__ out) {
    __builtin_amdgcn_s_setprio(3);   // beside another MSM's accumulation (overlap mode) the tail goes first
    const bool col = blockIdx.x >= row_blocks;
    const size_t t = ((size_t)(blockIdx.x - (col ? row_blocks : 0u)) * 64 + threadIdx.x) / RED_LANES;
    const uint32_t C = 1u << h, R = B >> h;
    const uint32_t q = col ? q_col : q_row, len = col ? R : C;
    const uint32_t g = len / q;                      // lanes per sum, 1 .. RED_FOLD
    const uint32_t nout = col ? C : R + 1;
    const size_t per_w = (size_t)nout * g;
    const size_t w = t / per_w;
    const uint32_t rem = (uint32_t)(t % per_w), o = rem / g, j = rem % g;
    const bool valid = w < (size_t)W;
    rec_sum sum;
    rec_sum_init(sum);
    if (valid) {
        const uint32_t* bk = buckets + w * (size_t)B * ZZS;
        for (uint32_t i = 0; i < q; ++i) {
            const uint32_t idx = j * q + i;
            const uint64_t b1 = col ? (uint64_t)idx * C + o : (uint64_t)o * C + idx;   // weight b + 1
            if (b1 >= 1 && b1 <= B) rec_sum_add(sum, bk + (size_t)(b1 - 1) * ZZS);
        }
    }
    rec_sum_fold(sum, g);
    Xyzz<ER> xa;
    rec_sum_get(xa, sum);
    Jac<ER> p;
    xyzz_to_jac(p, xa);
    if (valid && j == 0) store_jac(out + (w * (size_t)(R + 1 + C) + (col ? R + 1 + o : o)) * XYZW, p);
}

// rc[w]: R + 1 row sums, then C column sums (k_bucket_sums); planes[w][k], k < c
__global__ void __launch_bounds__(256) k_plane_sums(const uint32_t* __restrict__ rc, int W, int c, int h,
                                                     uint32_t* __restrict__ planes) {
    __shared__ uint32_t part[4 * XYZW];
    __builtin_amdgcn_s_setprio(3);
    const uint32_t w = blockIdx.x / (uint32_t)c, k = blockIdx.x % (uint32_t)c;
    const uint32_t C = 1u << h, R = (1u << (c - 1)) >> h, NP = R + 1 + C;
    const bool from_cols = k < (uint32_t)h;
    const uint32_t* src = rc + ((size_t)w * NP + (from_cols ? R + 1 : 0)) * XYZW;
    const uint32_t bit = from_cols ? k : k - (uint32_t)h;
    const bool top = k == (uint32_t)c - 1;            // weight B alone has this bit: row R
    const uint32_t M = top ? 1u : (from_cols ? C : R) / 2;
    const uint32_t nlanes = blockDim.x / RED_LANES, i0 = threadIdx.x / RED_LANES;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    Jac<ER> p, x;
    jac_set_inf(p);
    for (uint32_t i = i0; i < M; i += nlanes) {
        // i-th index with `bit` set
        const uint32_t idx = top ? R : (((i >> bit) << (bit + 1)) | (1u << bit) | (i & ((1u << bit) - 1u)));
        load_jac(x, src + (size_t)idx * XYZW);
        jac_add(p, p, x);
    }
    wave_group_sum_r(p, RED_FOLD);
    if (lane < (uint32_t)RED_LANES) store_jac(part + wave * XYZW, p);
    __syncthreads();
    if (wave != 0) return;
    const uint32_t jw = lane / RED_LANES;
    if (jw < nw) load_jac(p, part + jw * XYZW); else jac_set_inf(p);
    uint32_t G = 1;
    while (G < nw) G <<= 1;
    wave_group_sum_r(p, G);
    if (lane < (uint32_t)RED_LANES) store_jac(planes + ((size_t)w * c + k) * XYZW, p);
}

// The same with the last levels on lane-split elements (as k_sum_block_wide): every reduction lane adds its
// strided share of the plane's inputs, groups of four lanes fold per lane (two levels), the partial sums go to
// LDS and the waves of the workgroup halve them round by round, one lane-split addition at a time.
__global__ void __launch_bounds__(SUMW_THREADS) k_plane_sums_wide(const uint32_t* __restrict__ rc, int W, int c, int h,
                                                                  uint32_t* __restrict__ planes) {
    __shared__ uint32_t buf[2][SUMW_SLOTS * XYZW];
    __builtin_amdgcn_s_setprio(3);
    const uint32_t w = blockIdx.x / (uint32_t)c, k = blockIdx.x % (uint32_t)c;
    const uint32_t C = 1u << h, R = (1u << (c - 1)) >> h, NP = R + 1 + C;
    const bool from_cols = k < (uint32_t)h;
    const uint32_t* src = rc + ((size_t)w * NP + (from_cols ? R + 1 : 0)) * XYZW;
    const uint32_t bit = from_cols ? k : k - (uint32_t)h;
    const bool top = k == (uint32_t)c - 1;
    const uint32_t M = top ? 1u : (from_cols ? C : R) / 2;
    constexpr uint32_t NLANES = SUMW_THREADS / RED_LANES, NWAVES = SUMW_THREADS / 64;
    const uint32_t i0 = threadIdx.x / RED_LANES, wave = threadIdx.x >> 6;
    Jac<ER> p, x;
    jac_set_inf(p);
    for (uint32_t i = i0; i < M; i += NLANES) {
        const uint32_t idx = top ? R : (((i >> bit) << (bit + 1)) | (1u << bit) | (i & ((1u << bit) - 1u)));
        load_jac(x, src + (size_t)idx * XYZW);
        jac_add(p, p, x);
    }
    wave_group_sum_r(p, 4);
    if ((i0 & 3u) == 0) store_jac(buf[0] + (size_t)(i0 >> 2) * XYZW, p);
    __syncthreads();
    const WideEnv<FQ> env = wide_env<FQ>();
    uint32_t K = ((M < NLANES ? M : NLANES) + 3) / 4;   // partial sums: a power of two, or 1
    int cur = 0;
    while (K > 1) {
        const uint32_t pairs = K / 2;
        for (uint32_t q = wave; q < pairs; q += NWAVES) {   // wave-uniform
            const uint32_t* a = buf[cur] + (size_t)(2 * q) * XYZW;
            sum_wide_add(env, a, a + XYZW, buf[cur ^ 1] + (size_t)q * XYZW);
        }
        __syncthreads();
        cur ^= 1;
        K = pairs;
    }
    for (uint32_t t = threadIdx.x; t < (uint32_t)XYZW; t += SUMW_THREADS) planes[((size_t)w * c + k) * XYZW + t] = buf[cur][t];
}

// Horner over the window sums, high to low, c doublings between windows (multiexp.tcc:612-629),
// by one wave.  Prime-field groups with N < 16 limbs run the whole chain on lane-split
// coordinates (wide.cuh: one limb per lane, four products per step in the four DPP rows, ~3x
// fewer dependent instructions per doubling); the others share the products of a doubling
// among three lanes (jac_dbl_lanes3) with every lane holding the running point.
// init: running value handed over by the windows above this group (may be null).
template <class P, bool I>
AMDMSM_DEV typename std::enable_if<(P::N < 16), void>::type horner_chain(Jac<Fp<P, I>>& res,
                                                                         const uint32_t* __restrict__ window_sums, int W,
                                                                         int c, const uint32_t* __restrict__ init) {
    const WideEnv<P> env = wide_env<P>();
    auto load = [&](const uint32_t* p, uint32_t& X, uint32_t& Y, uint32_t& Z) {
        X = env.valid ? p[env.j] : 0u;
        Y = env.valid ? p[EW + env.j] : 0u;
        Z = env.valid ? p[2 * EW + env.j] : 0u;
    };
    uint32_t X, Y, Z, X2, Y2, Z2;
    int w = W - 1;
    if (init) {
        load(init, X, Y, Z);
    } else {
        load(window_sums + (size_t)w * XYZW, X, Y, Z);
        --w;
    }
    for (; w >= 0; --w) {
        if (!wide_is_zero(Z)) {
            // the c doublings as one run on 28-bit limbs with lazy linear operations (wide28.cuh:
            // 0.99 instead of 1.82 us each); very short runs do not repay the two conversions
            // (a != 0: the doublings of wide.cuh, jac_dbl_run28 is written for a = 0)
            if constexpr (GP::COEFF_A != 0) for (int i = 0; i < c; ++i) jac_dbl_wide<P, GP::COEFF_A>(env, X, Y, Z);
            else if (c >= 4) jac_dbl_run28<P>(env, X, Y, Z, c);
            else for (int i = 0; i < c; ++i) jac_dbl_wide<P>(env, X, Y, Z);
        }
        load(window_sums + (size_t)w * XYZW, X2, Y2, Z2);
        jac_add_wide<P, GP::COEFF_A>(env, X, Y, Z, X2, Y2, Z2);
    }
    wide_to_packed(res.x, X);
    wide_to_packed(res.y, Y);
    wide_to_packed(res.z, Z);
}
// prime fields of 16..31 limbs (bw6_761): two 32-lane rows, one product at a time
template <class P, bool I>
AMDMSM_DEV typename std::enable_if<(P::N >= 16 && P::N < 32), void>::type horner_chain(
    Jac<Fp<P, I>>& res, const uint32_t* __restrict__ window_sums, int W, int c, const uint32_t* __restrict__ init) {
    using F = WideFq<P>;
    const WideEnv<P> env = wide_env<P>();
    auto load = [&](const uint32_t* p, uint32_t& X, uint32_t& Y, uint32_t& Z) {
        X = env.valid ? p[env.j] : 0u;
        Y = env.valid ? p[EW + env.j] : 0u;
        Z = env.valid ? p[2 * EW + env.j] : 0u;
    };
    uint32_t X, Y, Z, X2, Y2, Z2;
    int w = W - 1;
    if (init) {
        load(init, X, Y, Z);
    } else {
        load(window_sums + (size_t)w * XYZW, X, Y, Z);
        --w;
    }
    for (; w >= 0; --w) {
        if (!wide_is_zero(Z)) {
            if (c >= 4) jac_dbl_run28<P>(env, X, Y, Z, c);   // 28 limbs of 28 bits, lazy linear operations
            else for (int i = 0; i < c; ++i) jac_dbl_wide2<P>(env, X, Y, Z);   // two products per round
        }
        load(window_sums + (size_t)w * XYZW, X2, Y2, Z2);
        jac_add_seq<F, P>(env, X, Y, Z, X2, Y2, Z2);
    }
    wide_to_packed(res.x, X);
    wide_to_packed(res.y, Y);
    wide_to_packed(res.z, Z);
}
// Fq2 groups: c0 / c1 in alternating rows, the three Karatsuba products of a multiplication side
// by side (WideFq2)
template <class P, int NR, bool I>
AMDMSM_DEV typename std::enable_if<(P::N < 16), void>::type horner_chain(Jac<Fp2<P, NR, I>>& res,
                                                                         const uint32_t* __restrict__ window_sums, int W,
                                                                         int c, const uint32_t* __restrict__ init) {
    using F = WideFq2<P, NR>;
    const WideEnv<P> env = wide_env<P>();
    const uint32_t wi = F::word_index(env);
    auto load = [&](const uint32_t* p, uint32_t& X, uint32_t& Y, uint32_t& Z) {
        X = env.valid ? p[wi] : 0u;
        Y = env.valid ? p[EW + wi] : 0u;
        Z = env.valid ? p[2 * EW + wi] : 0u;
    };
    uint32_t X, Y, Z, X2, Y2, Z2;
    int w = W - 1;
    if (init) {
        load(init, X, Y, Z);
    } else {
        load(window_sums + (size_t)w * XYZW, X, Y, Z);
        --w;
    }
    for (; w >= 0; --w) {
        if (!wide_is_zero(Z)) {
            // runs of doublings on 28-bit limbs with lazy linear operations (wide28.cuh)
            // (a != 0: jac_dbl_run28q is written for a = 0)
            if constexpr (GP::COEFF_A != 0) for (int i = 0; i < c; ++i) jac_dbl_seq<F, P, GP::COEFF_A>(env, X, Y, Z);
            else if (c >= 4) jac_dbl_run28q<P, NR>(env, X, Y, Z, c);
            else for (int i = 0; i < c; ++i) jac_dbl_seq<F, P>(env, X, Y, Z);
        }
        load(window_sums + (size_t)w * XYZW, X2, Y2, Z2);
        jac_add_seq<F, P, GP::COEFF_A>(env, X, Y, Z, X2, Y2, Z2);
    }
    wide_to_packed(res.x.c0, from_row(X, 0));
    wide_to_packed(res.x.c1, from_row(X, 1));
    wide_to_packed(res.y.c0, from_row(Y, 0));
    wide_to_packed(res.y.c1, from_row(Y, 1));
    wide_to_packed(res.z.c0, from_row(Z, 0));
    wide_to_packed(res.z.c1, from_row(Z, 1));
}
template <class EE>
AMDMSM_DEV void horner_chain(Jac<EE>& res, const uint32_t* __restrict__ window_sums, int W, int c,
                             const uint32_t* __restrict__ init, ...) {
    Jac<EE> x;
    int w = W - 1;
    if (init) {
        load_jac(res, init);
    } else {
        load_jac(res, window_sums + (size_t)w * XYZW);
        --w;
    }
    for (; w >= 0; --w) {
        for (int i = 0; i < c; ++i) jac_dbl_lanes3(res);
        load_jac(x, window_sums + (size_t)w * XYZW);
        jac_add(res, res, x);
    }
}

// The same chain, all of it on the loose 28-bit limbs of wide28.cuh (prime field, N < 16, a = 0): every loaded point is
// converted once (row r reads coordinate r, one product converts the three), the doublings (jac_dbl_28, runs of any
// length) and the additions (jac_add_28) stay loose, and one conversion at the end gives the canonical words the
// chain above produces.  The next window's point is loaded and converted before the doublings it does not depend on.
// Z of a converted point and of a sum is all-zero exactly at infinity (jac_add_28), so the test that skips the
// doublings is the one of the chain above.
constexpr bool HORNER_LAZY_OK = GP::DEG == 1 && FQ::N < 16 && GP::COEFF_A == 0;
template <class P, bool I>
AMDMSM_DEV void horner_chain_lazy(Jac<Fp<P, I>>& res, const uint32_t* __restrict__ window_sums, int W, int c,
                                  const uint32_t* __restrict__ init) {
    const WideEnv<P> env = wide_env<P>();
    const Env28<P, 10> v = env28<P, 10>(env);
    const uint32_t sub4 = tab28_sel(A28<P>::SUB4, env.j);
    const uint32_t row = (threadIdx.x & 63u) >> 4;
    auto load = [&](const uint32_t* p, uint32_t& X, uint32_t& Y, uint32_t& Z) {
        const uint32_t r = to28(v, (env.valid && row < 3u) ? p[row * EW + env.j] : 0u);
        X = from_row(r, 0);
        Y = from_row(r, 1);
        Z = from_row(r, 2);
    };
    uint32_t X, Y, Z, X2, Y2, Z2;
    int w = W - 1;
    if (init) {
        load(init, X, Y, Z);
    } else {
        load(window_sums + (size_t)w * XYZW, X, Y, Z);
        --w;
    }
    for (; w >= 0; --w) {
        load(window_sums + (size_t)w * XYZW, X2, Y2, Z2);
        if (!wide_is_zero(Z)) for (int i = 0; i < c; ++i) jac_dbl_28<P>(v, X, Y, Z);
        jac_add_28<P>(v, sub4, X, Y, Z, X2, Y2, Z2);
    }
    // Z may be twice a product (limbs up to 2^29 + 2^6): still a product operand
    const uint32_t r = from28(v, row == 0 ? X : (row == 1 ? Y : Z));
    wide_to_packed(res.x, from_row(r, 0));
    wide_to_packed(res.y, from_row(r, 1));
    wide_to_packed(res.z, from_row(r, 2));
}
// AMDMSM_HORNER_LAZY=0: the canonical chain (read once per process)
inline bool horner_lazy() {
    static const bool on = HORNER_LAZY_OK && !(getenv("AMDMSM_HORNER_LAZY") && atoi(getenv("AMDMSM_HORNER_LAZY")) == 0);
    return on;
}

__global__ void __launch_bounds__(64) k_horner(const uint32_t* __restrict__ window_sums, int W, int c, int form,
                                               const uint32_t* __restrict__ init, uint32_t* __restrict__ out) {
    __builtin_amdgcn_s_setprio(3);
    Jac<E> res;
    horner_chain(res, window_sums, W, c, init);
    if (threadIdx.x == 0) store_out(out, res, form);
}
// the kernels of the lazy chain are templates so that only the groups that launch them carry them
template <class EE = E>
__global__ void __launch_bounds__(64) k_horner_lazy(const uint32_t* __restrict__ window_sums, int W, int c, int form,
                                                    const uint32_t* __restrict__ init, uint32_t* __restrict__ out) {
    __builtin_amdgcn_s_setprio(3);
    Jac<EE> res;
    horner_chain_lazy(res, window_sums, W, c, init);
    if (threadIdx.x == 0) store_out(out, res, form);
}

// window sum = sum_k 2^k planes[w][k].  One workgroup per window: wave j folds planes 4j .. 4j+3 (Horner with one
// doubling between planes), then the first wave folds the ceil(c / 4) group values with four doublings between
// them -- a dependent chain of 3 + ceil(c / 4) additions instead of c - 1.
constexpr int WH_MAX_GROUPS = 6;   // c <= 24
__global__ void __launch_bounds__(64 * WH_MAX_GROUPS) k_window_horner(const uint32_t* __restrict__ planes, int c,
                                                                       uint32_t* __restrict__ out) {
    __shared__ uint32_t grp[WH_MAX_GROUPS * XYZW];
    __builtin_amdgcn_s_setprio(3);
    const int wave = (int)(threadIdx.x >> 6), ng = (c + 3) / 4;
    Jac<E> res;
    if (wave < ng) {
        const int k0 = 4 * wave, cnt = (c - k0 < 4) ? c - k0 : 4;
        horner_chain(res, planes + ((size_t)blockIdx.x * c + k0) * XYZW, cnt, 1, nullptr);
        if ((threadIdx.x & 63u) == 0) store_jac(grp + wave * XYZW, res);
    }
    __syncthreads();
    if (wave != 0) return;
    horner_chain(res, grp, ng, 4, nullptr);
    if (threadIdx.x == 0) store_jac(out + (size_t)blockIdx.x * XYZW, res);
}
template <class EE = E>
__global__ void __launch_bounds__(64 * WH_MAX_GROUPS) k_window_horner_lazy(const uint32_t* __restrict__ planes, int c,
                                                                            uint32_t* __restrict__ out) {
    __shared__ uint32_t grp[WH_MAX_GROUPS * XYZW];
    __builtin_amdgcn_s_setprio(3);
    const int wave = (int)(threadIdx.x >> 6), ng = (c + 3) / 4;
    Jac<EE> res;
    if (wave < ng) {
        const int k0 = 4 * wave, cnt = (c - k0 < 4) ? c - k0 : 4;
        horner_chain_lazy(res, planes + ((size_t)blockIdx.x * c + k0) * XYZW, cnt, 1, nullptr);
        if ((threadIdx.x & 63u) == 0) store_jac(grp + wave * XYZW, res);
    }
    __syncthreads();
    if (wave != 0) return;
    horner_chain_lazy(res, grp, ng, 4, nullptr);
    if (threadIdx.x == 0) store_jac(out + (size_t)blockIdx.x * XYZW, res);
}

// k Horner chains at once (amdmsm_msm_device_batch): block j folds the W window sums of MSM j
struct horner_outs {
    uint32_t* p[8];
};
__global__ void __launch_bounds__(64) k_horner_batch(const uint32_t* __restrict__ window_sums, int W, int c, int form,
                                                     horner_outs outs) {
    __builtin_amdgcn_s_setprio(3);
    Jac<E> res;
    horner_chain(res, window_sums + (size_t)blockIdx.x * W * XYZW, W, c, nullptr);
    uint32_t* out = outs.p[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) out = (blockIdx.x == (unsigned)j) ? outs.p[j] : out;
    if (threadIdx.x == 0) store_out(out, res, form);
}
template <class EE = E>
__global__ void __launch_bounds__(64) k_horner_batch_lazy(const uint32_t* __restrict__ window_sums, int W, int c, int form,
                                                          horner_outs outs) {
    __builtin_amdgcn_s_setprio(3);
    Jac<EE> res;
    horner_chain_lazy(res, window_sums + (size_t)blockIdx.x * W * XYZW, W, c, nullptr);
    uint32_t* out = outs.p[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) out = (blockIdx.x == (unsigned)j) ? outs.p[j] : out;
    if (threadIdx.x == 0) store_out(out, res, form);
}

// plain sum of k engine-Jacobian points by one wave: the Horner chain with no doublings, i.e. on
// lane-split coordinates (partials of chunked / multi-GPU calls, multiexp.tcc:681-687)
__global__ void __launch_bounds__(64) k_sum_points(const uint32_t* __restrict__ pts, int k, int form,
                                                   uint32_t* __restrict__ out) {
    Jac<E> res;
    if (k <= 0) jac_set_inf(res);
    else horner_chain(res, pts, k, 0, nullptr);
    if (threadIdx.x == 0) store_out(out, res, form);
}

// ------------------------------------------------------------ base import
// libff (X, Y, Z) records -> compact affine.  Special form: copy.  Normal form: one lane takes
// IMPORT_K consecutive points and shares a single field inversion among them (Montgomery's
// trick, as batch_to_special / batch_invert do on the host: multiexp.tcc:949-974,
// field_utils.tcc:419-439); prefix products are parked in the output slots between the two
// passes.  Lanes whose points all have Z == 1 already (the usual case: default BaseForm on an
// affine proving key) skip the inversion.
constexpr int IMPORT_K = 32;

__global__ void __launch_bounds__(TPB) k_import_bases(const uint32_t* __restrict__ src, size_t stride_words,
                                                      int form_special, size_t n, uint32_t* __restrict__ dst) {
    if (form_special) {
        const size_t i = gtid();
        if (i >= n) return;
        const uint32_t* q = src + i * stride_words;
        // Z == 1 or the element is zero (is_special, alt_bn128_g1.cpp:86-89)
        Aff<E> a;
        E z;
        el_load(a.x, q);
        el_load(a.y, q + EW);
        el_load(z, q + 2 * EW);
        if (el_is_zero(z)) {
            el_zero(a.x);
            el_zero(a.y);
        }
        store_aff(dst + i * AFFW, a);
        return;
    }
    const size_t i0 = gtid() * IMPORT_K;
    if (i0 >= n) return;
    const size_t i1 = (i0 + IMPORT_K < n) ? i0 + IMPORT_K : n;
    E one, acc;
    el_one(one);
    acc = one;
    bool trivial = true;
    for (size_t i = i0; i < i1; ++i) {
        Jac<E> p;
        load_libff(p, src + i * stride_words);
        if (jac_is_inf(p)) continue;
        el_store(dst + i * AFFW, acc);   // prefix product of the Z's before this point
        if (!el_eq(p.z, one)) {
            trivial = false;
            el_mul(acc, acc, p.z);
        }
    }
    E inv = one;
    if (!trivial) el_inv(inv, acc);
    for (size_t i = i1; i-- > i0;) {
        Jac<E> p;
        load_libff(p, src + i * stride_words);
        Aff<E> a;
        if (jac_is_inf(p)) {
            el_zero(a.x);
            el_zero(a.y);
        } else if (el_eq(p.z, one)) {
            a.x = p.x;
            a.y = p.y;
        } else {
            E pre, zi, z2;
            el_load(pre, dst + i * AFFW);
            el_mul(zi, inv, pre);      // Z_i^-1
            el_mul(inv, inv, p.z);
            el_sqr(z2, zi);
            el_mul(a.x, p.x, z2);
            el_mul(z2, z2, zi);
            el_mul(a.y, p.y, z2);
        }
        store_aff(dst + i * AFFW, a);
    }
}

__global__ void __launch_bounds__(TPB) k_export_affine(const uint32_t* __restrict__ src, size_t n,
                                                       uint32_t* __restrict__ dst) {
    const size_t i = gtid();
    if (i >= n) return;
    Aff<E> a;
    load_aff(a, src + i * AFFW);
    Jac<E> p;
    jac_from_aff(p, a);
    store_jac(dst + i * XYZW, p);
}

// Table of precomputed multiples for the single-bucket-set MSM (what profile_multiexp.cpp:120-150
// writes to disk for multi_exp_stream_with_precompute): table[i*D + j] = [2^(j*c)] P_i, affine.
// One lane walks one base through (D-1)*c doublings; (X, Y) are parked in the table slots and
// (Z, prefix product of the Z's) in tmp, then one inversion per lane turns all D entries affine.
#if AMDMSM_ACC_RR
// The doubling chain of one table row on reduced-radix limbs (groups with coordinates in Fq): (D - 1) c doublings with the
// squarings the 32-bit words cannot afford, (X, Y, Z) exported to canonical words every c doublings for the shared inversion
// that follows.  Returns false where it does not apply (the caller then runs the 32-bit chain).
template <class G, class A, class EL>   // G = GP, A = Aff<E>, EL = E: template parameters keep the Fq2 groups from instantiating the body
AMDMSM_DEV bool precompute_chain_rr(const A& a, int c, int D, uint32_t* row, uint32_t* trow, EL& acc, int& last) {
    if constexpr (G::DEG == 1) {
        using FQL = typename G::fq;
        using R = Rr<FQL>;
        uint32_t wx[FQL::N], wy[FQL::N];
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < FQL::N; ++j) {
            wx[j] = a.x.v[j];
            wy[j] = a.y.v[j];
            any |= wx[j] | wy[j];
        }
        JacRr<R> cur;
        re_from_words_rho(cur.x, wx);
        re_from_words_rho(cur.y, wy);
        re_set_pow2<rr_shape<FQL>::B * rr_shape<FQL>::L>(cur.z);   // one
        bool inf = any == 0;
        for (int j = 1; j < D; ++j) {
#pragma nounroll
            for (int k = 0; k < c; ++k) jac_dbl_rr(cur, inf);
            if (jac_is_inf_rr(cur, inf)) break;
            EL x, y, z;
            rr_export_component<FQL, 0>(x.v, cur.x);
            rr_export_component<FQL, 0>(y.v, cur.y);
            rr_export_component<FQL, 0>(z.v, cur.z);
            el_store(row + (size_t)j * AFFW, x);
            el_store(row + (size_t)j * AFFW + EW, y);
            el_store(trow + (size_t)j * AFFW, z);
            el_store(trow + (size_t)j * AFFW + EW, acc);
            el_mul(acc, acc, z);
            last = j;
        }
        return true;
    } else {
        return false;
    }
}
#endif

__global__ void __launch_bounds__(TPB) k_precompute_table(const uint32_t* __restrict__ bases, size_t n, int c, int D,
                                                          uint32_t* __restrict__ tmp, uint32_t* __restrict__ table) {
    const size_t i = gtid();
    if (i >= n) return;
    Aff<E> a;
    load_aff(a, bases + i * AFFW);
    uint32_t* row = table + i * (size_t)D * AFFW;
    uint32_t* trow = tmp + i * (size_t)D * AFFW;   // per entry: Z, prefix
    store_aff(row, a);
    E acc;
    el_one(acc);
    int last = 0;   // entries 1 .. last are finite (an infinite base or a point of even order stops early)
#if AMDMSM_ACC_RR
    if (precompute_chain_rr<GP>(a, c, D, row, trow, acc, last)) {
    } else
#endif
    {
        Jac<E> cur;
        jac_from_aff(cur, a);
        for (int j = 1; j < D; ++j) {
            for (int k = 0; k < c; ++k) jac_dbl(cur, cur);
            if (jac_is_inf(cur)) break;
            el_store(row + (size_t)j * AFFW, cur.x);
            el_store(row + (size_t)j * AFFW + EW, cur.y);
            el_store(trow + (size_t)j * AFFW, cur.z);
            el_store(trow + (size_t)j * AFFW + EW, acc);
            el_mul(acc, acc, cur.z);
            last = j;
        }
    }
    E inv;
    el_inv(inv, acc);
    for (int j = D - 1; j >= 1; --j) {
        Aff<E> o;
        if (j > last) {
            el_zero(o.x);
            el_zero(o.y);
        } else {
            E z, pre, zi, z2, x, y;
            el_load(z, trow + (size_t)j * AFFW);
            el_load(pre, trow + (size_t)j * AFFW + EW);
            el_load(x, row + (size_t)j * AFFW);
            el_load(y, row + (size_t)j * AFFW + EW);
            el_mul(zi, inv, pre);   // Z_j^-1
            el_mul(inv, inv, z);
            el_sqr(z2, zi);
            el_mul(o.x, x, z2);
            el_mul(z2, z2, zi);
            el_mul(o.y, y, z2);
        }
        store_aff(row + (size_t)j * AFFW, o);
    }
}

AMDMSM_DEV void load_generator(Jac<E>& g) {
    el_set_words(g.x, GP::GEN_X);
    el_set_words(g.y, GP::GEN_Y);
    el_one(g.z);
}

__global__ void __launch_bounds__(TPB) k_gen_bases_seq(unsigned long long first, size_t n, uint32_t* __restrict__ dst) {
    const size_t i = gtid();
    if (i >= n) return;
    Jac<E> g, r;
    load_generator(g);
    jac_mul_u64(r, g, first + i + 1ull);
    Aff<E> a;
    jac_to_aff(a, r);
    store_aff(dst + i * AFFW, a);
}

// ------------------------------------------------------------ on-disk bases
// libff's binary, Montgomery, uncompressed group-element records (what multi_exp_stream reads,
// multiexp_stream.tcc:19-49; writer group_element_codec<encoding_binary, Form, compression_off>,
// curve_serialization.tcc:78-101): affine X || Y; every Fq component is the Montgomery residue
// with its bytes reversed (big-endian; field_serialization.tcc:197-223), extension
// coefficients in ascending order c0, c1 (field_serialization.tcc:124-146); zero = (0, one).
template <bool I>
AMDMSM_DEV void load_be_raw(Fp<FQ, I>& r, const uint32_t* __restrict__ src) {
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) r.v[j] = bswap32(src[FQ::N - 1 - j]);
}
template <bool I>
AMDMSM_DEV void load_coord_disk(Fp<FQ, I>& r, const uint32_t* src) { load_be_raw(r, src); }
template <int NR, bool I>
AMDMSM_DEV void load_coord_disk(Fp2<FQ, NR, I>& r, const uint32_t* src) {
    load_be_raw(r.c0, src);
    load_be_raw(r.c1, src + FQ::N);
}

__global__ void __launch_bounds__(TPB) k_disk_decode(const uint32_t* __restrict__ src, size_t n, uint32_t* __restrict__ dst) {
    const size_t i = gtid();
    if (i >= n) return;
    Aff<E> a;
    load_coord_disk(a.x, src + i * AFFW);
    load_coord_disk(a.y, src + i * AFFW + EW);
    E one;
    el_one(one);
    if (el_is_zero(a.x) && el_eq(a.y, one)) el_zero(a.y);   // (0, one) is zero (curve_serialization.tcc:95-99)
    store_aff(dst + i * AFFW, a);
}

// Compressed records (group_element_codec<encoding_binary, form_montgomery, compression_on>,
// curve_serialization.tcc:103-166): X only -- for Fq2 its component c0 first, then c1 -- each
// component big-endian, with two flag bits in the top of the first component's highest limb
// (field_serialization.tcc:186-266: FLAG_SHIFT = 62): bit 0 = lowest bit of Y.c0's Montgomery
// representation, bit 1 = the element is zero.  Y = sqrt(X^3 + b) (curve_point_y_at_x,
// curve_utils.tcc:34-47), negated when its low bit disagrees with the flag.  status |= 2 where
// X^3 + b has no square root (the reference's sqrt does not terminate on such input).
template <bool I>
AMDMSM_DEV const Fp<FQ, I>& coord_c0(const Fp<FQ, I>& a) { return a; }
template <int NR, bool I>
AMDMSM_DEV const Fp<FQ, I>& coord_c0(const Fp2<FQ, NR, I>& a) { return a.c0; }

__global__ void __launch_bounds__(64) k_disk_decode_compressed(const uint32_t* __restrict__ src, size_t n,
                                                                 uint32_t* __restrict__ dst, uint32_t* __restrict__ status) {
    const size_t i = gtid();
    if (i >= n) return;
    const uint32_t* q = src + i * EW;
    const uint32_t flags = bswap32(q[0]) >> 30;
    Aff<E> a;
    load_coord_disk(a.x, q);
    reinterpret_cast<uint32_t*>(&a.x)[FQ::N - 1] &= 0x3fffffffu;   // top limb of component 0 carries the flags
    if (flags & 2u) {
        el_zero(a.x);
        el_zero(a.y);
    } else {
        E y2, b;
        el_sqr(y2, a.x);
        el_mul(y2, y2, a.x);
        el_set_words(b, GP::COEFF_B);
        el_add(y2, y2, b);
        if (!el_sqrt(a.y, y2)) atomicOr(status, 2u);
        if ((coord_c0(a.y).v[0] & 1u) != (flags & 1u)) el_neg(a.y, a.y);
    }
    store_aff(dst + i * AFFW, a);
}

// The writers of the same two record forms (group_write<encoding_binary, form_montgomery, compression_{off,on}>,
// curve_serialization.tcc:78-133), the inverses of the two decoders above: compact affine records in, one lane per
// record, the lanes of a wave on consecutive records and the grid striding over the vector.  Every index comes from n and
// the launch geometry.  flags: or-ed into the top two bits of the component's highest limb -- the first byte written.
template <bool I>
AMDMSM_DEV void store_be_raw(uint32_t* __restrict__ dst, const Fp<FQ, I>& a, uint32_t flags) {
    Fp<FQ, I> t;
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) t.v[j] = bswap32(a.v[FQ::N - 1 - j]);
    t.v[0] = bswap32(a.v[FQ::N - 1] | (flags << 30));
    fp_store(dst, t);
}
template <bool I>
AMDMSM_DEV void store_coord_disk(uint32_t* dst, const Fp<FQ, I>& a, uint32_t flags) { store_be_raw(dst, a, flags); }
template <int NR, bool I>
AMDMSM_DEV void store_coord_disk(uint32_t* dst, const Fp2<FQ, NR, I>& a, uint32_t flags) {
    store_be_raw(dst, a.c0, flags);
    store_be_raw(dst + FQ::N, a.c1, 0u);
}

// X || Y; the compact zero (0, 0) leaves as (0, one), what the reference writes after to_affine_coordinates on zero
__global__ void __launch_bounds__(TPB) k_disk_encode(const uint32_t* __restrict__ src, size_t n, uint32_t* __restrict__ dst) {
    const size_t step = (size_t)gridDim.x * TPB;
    for (size_t i = gtid(); i < n; i += step) {
        Aff<E> a;
        load_aff(a, src + i * AFFW);
        if (el_is_zero(a.x) && el_is_zero(a.y)) el_one(a.y);
        store_coord_disk(dst + i * AFFW, a.x, 0u);
        store_coord_disk(dst + i * AFFW + EW, a.y, 0u);
    }
}

// X only, flag bit 0 = the low bit of Y's (Y.c0's) Montgomery word 0, flag bit 1 = zero, which is written as X = 0 with
// that flag alone (curve_serialization.tcc:103-133 on G::zero()).  For the a = 0 curves, as the decoder.
__global__ void __launch_bounds__(TPB) k_disk_encode_compressed(const uint32_t* __restrict__ src, size_t n,
                                                                uint32_t* __restrict__ dst) {
    const size_t step = (size_t)gridDim.x * TPB;
    for (size_t i = gtid(); i < n; i += step) {
        Aff<E> a;
        load_aff(a, src + i * AFFW);
        const bool zero = el_is_zero(a.x) && el_is_zero(a.y);
        const uint32_t flags = zero ? 2u : (coord_c0(a.y).v[0] & 1u);
        store_coord_disk(dst + i * EW, a.x, flags);
    }
}

// ------------------------------------------------- fixed-base exponentiation
// batch_exp / batch_exp_with_coeff (multiexp.tcc:874-947): res[i] = v[i] * g through a window
// table powers_of_g[outer][inner] = inner * 2^(outer*window) * g (get_window_table,
// multiexp.tcc:809-846; the last row is shorter).  The reference builds each row with 2^window
// serial additions; here row `outer` grows by binary splitting -- entry j = 2 * entry[j/2]
// (+ gouter if j is odd), one launch per bit -- and the per-scalar loop (windowed_exp,
// multiexp.tcc:848-872) is one lane per scalar.
__global__ void __launch_bounds__(64) k_fb_gouter(const uint32_t* __restrict__ g_xyz, int outerc, int window,
                                                  uint32_t* __restrict__ gouter) {
    Jac<E> p;
    load_libff(p, g_xyz);
    for (int outer = 0; outer < outerc; ++outer) {
        if (threadIdx.x == 0) store_jac(gouter + (size_t)outer * XYZW, p);
        for (int i = 0; i < window; ++i) jac_dbl_lanes3(p);
    }
}

// level `bit` (0 = top bit of the window): fills entries [2^bit, 2^(bit+1)) of every row from
// entries [2^(bit-1), 2^bit); level 0 writes entries 0 (zero) and 1 (gouter).
__global__ void __launch_bounds__(TPB) k_fb_table_level(const uint32_t* __restrict__ gouter, int outerc, int window,
                                                        int scalar_size, int level, uint32_t* __restrict__ table) {
    const size_t t = gtid();
    const size_t row_len = (size_t)1 << window;
    const size_t per_level = level == 0 ? 2 : ((size_t)1 << level);
    const size_t outer = t / per_level;
    if (outer >= (size_t)outerc) return;
    const size_t j = level == 0 ? (t % per_level) : (per_level + t % per_level);
    // rows are 2^window long except the last: 2^(scalar_size - (outerc-1)*window) (multiexp.tcc:815)
    const size_t cur_len = (outer == (size_t)outerc - 1) ? ((size_t)1 << (scalar_size - (outerc - 1) * window)) : row_len;
    if (j >= cur_len) return;
    uint32_t* row = table + outer * row_len * XYZW;
    Jac<E> p, go;
    if (level == 0) {
        if (j == 0) jac_set_inf(p); else load_jac(p, gouter + outer * XYZW);
    } else {
        load_jac(p, row + (j >> 1) * XYZW);
        jac_dbl(p, p);
        if (j & 1) {
            load_jac(go, gouter + outer * XYZW);
            jac_add(p, p, go);
        }
    }
    store_jac(row + j * XYZW, p);
}

// The table made affine once (compact records, (0, 0) = zero), FB_NORM_K entries per lane sharing one
// inversion (Montgomery's trick, as k_import_bases): the per-scalar loop below then adds table entries
// with the mixed addition of the bucket accumulation (8M + 2S on XYZZ accumulators) instead of the full
// Jacobian addition with its equality pre-test (11M + 5S + 6M + 2S, alt_bn128_g1.cpp:164).
constexpr int FB_NORM_K = 32;
__global__ void __launch_bounds__(TPB) k_fb_table_affine(const uint32_t* __restrict__ table, size_t n, uint32_t* __restrict__ dst) {
    const size_t i0 = gtid() * FB_NORM_K;
    if (i0 >= n) return;
    const size_t i1 = (i0 + FB_NORM_K < n) ? i0 + FB_NORM_K : n;
    E acc;
    el_one(acc);
    for (size_t i = i0; i < i1; ++i) {
        Jac<E> p;
        load_jac(p, table + i * XYZW);
        if (jac_is_inf(p)) continue;
        el_store(dst + i * AFFW, acc);   // prefix product of the Z's before this entry
        el_mul(acc, acc, p.z);
    }
    E inv;
    el_inv(inv, acc);
    for (size_t i = i1; i-- > i0;) {
        Jac<E> p;
        load_jac(p, table + i * XYZW);
        Aff<E> a;
        if (jac_is_inf(p)) {
            el_zero(a.x);
            el_zero(a.y);
        } else {
            E pre, zi, z2;
            el_load(pre, dst + i * AFFW);
            el_mul(zi, inv, pre);      // Z_i^-1
            el_mul(inv, inv, p.z);
            el_sqr(z2, zi);
            el_mul(a.x, p.x, z2);
            el_mul(z2, z2, zi);
            el_mul(a.y, p.y, z2);
        }
        store_aff(dst + i * AFFW, a);
    }
}

// res[i] = (coeff *) v[i] * g (windowed_exp, multiexp.tcc:848-872): one lane per scalar, one mixed addition
// per nonzero window digit into an XYZZ accumulator, table entries affine
__global__ void __launch_bounds__(TPB) k_fb_exp(const uint32_t* __restrict__ table_aff, const uint32_t* __restrict__ scalars,
                                                size_t n, int mont, const uint32_t* __restrict__ coeff, int scalar_size,
                                                int window, int form, uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    Fp<FR> x;
    fp_load(x, scalars + i * FRW);
    if (coeff) {   // coeff * v[i] (batch_exp_with_coeff, multiexp.tcc:937)
        Fp<FR> cf;
        fp_load(cf, coeff);
        if (!mont) {
            fp_to_mont(x, x);
            fp_to_mont(cf, cf);
        }
        fp_mul(x, x, cf);
        fp_from_mont(x, x);
    } else if (mont) {
        fp_from_mont(x, x);
    }
    const int outerc = (scalar_size + window - 1) / window;
    const size_t row_len = (size_t)1 << window;
    const uint32_t wmask = (1u << window) - 1u;
    Xyzz<E> acc;
    Aff<E> e;
    xyzz_set_inf(acc);   // powers_of_g[0][0] = zero
    uint64_t buf = 0;
    int nbits = 0, outer = 0;
#pragma unroll
    for (int j = 0; j < FRW; ++j) {
        buf |= (uint64_t)x.v[j] << nbits;
        nbits += 32;
        while (nbits >= window && outer < outerc) {
            const uint32_t inner = (uint32_t)buf & wmask;
            buf >>= window;
            nbits -= window;
            if (inner) {
                load_aff(e, table_aff + ((size_t)outer * row_len + inner) * AFFW);
                xyzz_madd(acc, e);
            }
            ++outer;
        }
    }
    while (outer < outerc) {
        const uint32_t inner = (uint32_t)buf & wmask;
        buf >>= window;
        if (inner) {
            load_aff(e, table_aff + ((size_t)outer * row_len + inner) * AFFW);
            xyzz_madd(acc, e);
        }
        ++outer;
    }
    Jac<E> res;
    xyzz_to_jac(res, acc);
    store_out(out + i * XYZW, res, form);
}

// -------------------------------------------------------------- FFI codecs
// libff's FFI wire format (ffi/ffi_serialization.hpp:12-16, .tcc:19-187): every prime-field
// component is a big-endian plain (non-Montgomery) integer padded to the in-memory bigint
// size, extension coefficients highest-order first, points are affine X || Y, zero = (0, 1).

// one Fq component: BE bytes -> LE words; false when the value is not < modulus (:65-76)
template <bool I>
AMDMSM_DEV bool load_be_plain(Fp<FQ, I>& r, const uint32_t* __restrict__ src) {
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) r.v[j] = bswap32(src[FQ::N - 1 - j]);
    return fp_lt_modulus(r);
}
template <bool I>
AMDMSM_DEV void store_be_plain(uint32_t* __restrict__ dst, const Fp<FQ, I>& a) {
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) dst[FQ::N - 1 - j] = bswap32(a.v[j]);
}
template <bool I>
AMDMSM_DEV bool load_coord_be(Fp<FQ, I>& r, const uint32_t* src) { return load_be_plain(r, src); }
template <bool I>
AMDMSM_DEV void store_coord_be(uint32_t* dst, const Fp<FQ, I>& a) { store_be_plain(dst, a); }
template <int NR, bool I>
AMDMSM_DEV bool load_coord_be(Fp2<FQ, NR, I>& r, const uint32_t* src) {
    const bool ok1 = load_be_plain(r.c1, src);   // field_serializer: coeffs[degree-1] first (:25-36)
    const bool ok0 = load_be_plain(r.c0, src + FQ::N);
    return ok0 && ok1;
}
template <int NR, bool I>
AMDMSM_DEV void store_coord_be(uint32_t* dst, const Fp2<FQ, NR, I>& a) {
    store_be_plain(dst, a.c1);
    store_be_plain(dst + FQ::N, a.c0);
}

// bls12_377 G1: P + [c1] sigma(P) == 0, sigma(x, y) = (beta x, y) (bls12_377_g1.cpp:359-365, 387-397)
template <class G, int K = G::SUBGROUP_CHECK>
struct endo_check {
    static AMDMSM_DEV bool run(const Aff<E>&) { return true; }
};
template <class G>
struct endo_check<G, 2> {
    static AMDMSM_DEV bool run(const Aff<E>& a) {
        Jac<E> p, sg, t;
        jac_from_aff(p, a);
        E beta;
        el_set_words(beta, G::ENDO_BETA);
        sg = p;
        el_mul(sg.x, sg.x, beta);
        jac_mul_words<E, 4>(t, sg, G::ENDO_C1);
        jac_add(t, t, p);
        return jac_is_inf(t);
    }
};
template <class G>
AMDMSM_DEV bool endo_subgroup_check(const Aff<E>& a) { return endo_check<G>::run(a); }

// [a]P + [b]phi(P) == 0 with (a, b) = glv::SUB_*: a + b lambda = 0 (mod r) and a^2 - a b + b^2 = r, so for a curve
// point the test holds exactly when [r]P == 0 (tools/gen_params.py subgroup_vector) -- the reference's
// zero() == scalar_field::mod * P (bw6_761_g1.cpp:385-388, alt_bn128_g2.cpp:389-392, and bls12_377_g2.cpp:461-473 as
// decided on this curve) with scalars of half the length: one joint double-and-add over the non-adjacent forms of a
// and b (about 2/3 of a mixed addition per doubling instead of a full addition every second doubling of a scalar
// twice as long).  Every lane follows the same digits: no divergence.
template <bool I>
AMDMSM_DEV void scale_by_beta(Fp<FQ, I>& x) {
    Fp<FQ, I> beta;
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) beta.v[j] = GP::GLV_BETA[j];
    fp_mul(x, x, beta);
}
template <int NR, bool I>
AMDMSM_DEV void scale_by_beta(Fp2<FQ, NR, I>& x) {   // beta lies in Fq: both components are scaled
    scale_by_beta(x.c0);
    scale_by_beta(x.c1);
}
AMDMSM_DEV bool lattice_subgroup_check(const Aff<E>& a) {
    Aff<E> p1 = a, p2 = a, n1, n2;
    scale_by_beta(p2.x);   // phi(x, y) = (beta x, y)
    n1 = p1;
    n2 = p2;
    el_neg(n1.y, n1.y);
    el_neg(n2.y, n2.y);
    Jac<E> t;
    jac_set_inf(t);
    for (int i = GLV::SUB_BITS - 1; i >= 0; --i) {
        jac_dbl(t, t);
        const int wd = i >> 5;
        const uint32_t m = 1u << (i & 31);
        if (GLV::SUB_A_POS[wd] & m) jac_madd(t, p1);
        if (GLV::SUB_A_NEG[wd] & m) jac_madd(t, n1);
        if (GLV::SUB_B_POS[wd] & m) jac_madd(t, p2);
        if (GLV::SUB_B_NEG[wd] & m) jac_madd(t, n2);
    }
    return jac_is_inf(t);
}

#if AMDMSM_ACC_RR
// The same two tests on reduced-radix limbs (rr.cuh jac_dbl_rr / jac_madd_rr) for the groups with coordinates in Fq:
// the chains are 128-380 doublings long, every lane on the same scalar, and run at the multiply-issue rate.
template <class G>   // G = GP; templates so that the Fq2 groups do not instantiate them
AMDMSM_DEV bool endo_subgroup_check_rr(const uint32_t (&wx)[FQ::N], const uint32_t (&wy)[FQ::N]) {
    using R = Rr<typename G::fq>;
    R px, py, sx, beta;
    re_from_words_rho(px, wx);
    re_from_words_rho(py, wy);
    re_from_words_rho(beta, G::ENDO_BETA);
    re_mul(sx, px, beta);   // sigma(x, y) = (beta x, y)
    JacRr<R> t;
    rr_zero(t.x); rr_zero(t.y); rr_zero(t.z);
    bool inf = true;
    // one doubling and one addition in the code (each inlined copy costs registers: five sites put the kernel at one wave
    // per SIMD): the closing "+ P" is step -1 of the same loop
#pragma nounroll
    for (int i = 4 * 32 - 1; i >= -1; --i) {   // [c1] sigma(P), most significant bit first (curve_utils.tcc:14-32), then + P
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w = ((i >> 5) == j) ? G::ENDO_C1[j] : w;
        if (i >= 0) jac_dbl_rr(t, inf);
        if (i < 0 || ((w >> (i & 31)) & 1u)) {
            R ax;
#pragma unroll
            for (int k = 0; k < R::L; ++k) ax.v[k] = i < 0 ? px.v[k] : sx.v[k];
            jac_madd_rr(t, inf, ax, py);
        }
    }
    return jac_is_inf_rr(t, inf);
}
template <class G>
AMDMSM_DEV bool lattice_subgroup_check_rr(const uint32_t (&wx)[FQ::N], const uint32_t (&wy)[FQ::N]) {
    using R = Rr<typename G::fq>;
    R p1x, p2x, py, ny, beta;
    re_from_words_rho(p1x, wx);
    re_from_words_rho(py, wy);
    re_from_words_rho(beta, G::GLV_BETA);
    re_mul(p2x, p1x, beta);   // phi(x, y) = (beta x, y)
    re_neg(ny, py);
    re_norm(ny, ny);
    JacRr<R> t;
    rr_zero(t.x); rr_zero(t.y); rr_zero(t.z);
    bool inf = true;
    // one doubling and one addition in the code: the digits of a (part 0) and b (part 1) take turns in an inner loop
    // (non-adjacent forms: at most one of +-P and one of +-phi(P) per bit)
#pragma nounroll
    for (int i = GLV::SUB_BITS - 1; i >= 0; --i) {
        jac_dbl_rr(t, inf);
        const int wd = i >> 5;
        const uint32_t m = 1u << (i & 31);
#pragma nounroll
        for (int part = 0; part < 2; ++part) {
            const bool pos = ((part ? GLV::SUB_B_POS[wd] : GLV::SUB_A_POS[wd]) & m) != 0;
            const bool neg = ((part ? GLV::SUB_B_NEG[wd] : GLV::SUB_A_NEG[wd]) & m) != 0;
            if (pos || neg) {
                R ax, ay;
#pragma unroll
                for (int k = 0; k < R::L; ++k) {
                    ax.v[k] = part ? p2x.v[k] : p1x.v[k];
                    ay.v[k] = pos ? py.v[k] : ny.v[k];
                }
                jac_madd_rr(t, inf, ax, ay);
            }
        }
    }
    return jac_is_inf_rr(t, inf);
}
template <class G, class A>   // A = Aff<E>: a template parameter so that a.x.v is only looked up where DEG == 1
AMDMSM_DEV bool in_safe_subgroup_rr(const A& a, bool& done) {
    done = false;
    if constexpr (G::DEG == 1) {
#ifndef AMDMSM_SUBGROUP_BY_ORDER
        if constexpr (G::SUBGROUP_CHECK == 2 || G::SUBGROUP_CHECK == 3) {
            uint32_t wx[FQ::N], wy[FQ::N];
#pragma unroll
            for (int j = 0; j < FQ::N; ++j) {
                wx[j] = a.x.v[j];
                wy[j] = a.y.v[j];
            }
            done = true;
            if constexpr (G::SUBGROUP_CHECK == 2) return endo_subgroup_check_rr<G>(wx, wy);
            else return lattice_subgroup_check_rr<G>(wx, wy);
        }
#endif
    }
    return false;
}
#endif

AMDMSM_DEV bool in_safe_subgroup(const Aff<E>& a) {
    if (GP::SUBGROUP_CHECK == 0) return true;   // alt_bn128_g1.cpp:359-363
#if AMDMSM_ACC_RR
    {
        bool done;
        const bool ok = in_safe_subgroup_rr<GP>(a, done);
        if (done) return ok;
    }
#endif
#ifndef AMDMSM_SUBGROUP_BY_ORDER
    if (GP::SUBGROUP_CHECK == 3) return lattice_subgroup_check(a);
#endif
    Jac<E> p, t;
    jac_from_aff(p, a);
    if (GP::SUBGROUP_CHECK == 1 || GP::SUBGROUP_CHECK == 3) {   // zero() == scalar_field::mod * P (bw6_761_g1.cpp:385-388)
        jac_mul_words<E, FRW>(t, p, FR::P);
        return jac_is_inf(t);
    }
    return endo_subgroup_check<GP>(a);
}

// status bits: 1 = coordinate out of range, 2 = not on the curve, 4 = not in the safe subgroup
#ifndef AMDMSM_FFI_WAVES
#define AMDMSM_FFI_WAVES ((AMDMSM_ACC_RR && GP::DEG == 1 && FQ::N <= 12) ? 2 : 1)
#endif
__global__ void __launch_bounds__(TPB, AMDMSM_FFI_WAVES) k_ffi_decode_points(const uint32_t* __restrict__ src, size_t n,
                                                           uint32_t* __restrict__ dst, uint32_t* __restrict__ status) {
    const size_t i = gtid();
    if (i >= n) return;
    const uint32_t* q = src + i * AFFW;
    Aff<E> a;
    const bool okx = load_coord_be(a.x, q);
    const bool oky = load_coord_be(a.y, q + EW);
    uint32_t bad = (okx && oky) ? 0u : 1u;
    E one_plain;
    el_zero(one_plain);
    reinterpret_cast<uint32_t*>(&one_plain)[0] = 1u;
    if (el_is_zero(a.x) && el_eq(a.y, one_plain)) {
        el_zero(a.x);   // (0, 1) encodes zero (group_element_read, :158-163)
        el_zero(a.y);
    } else if (!bad) {
        el_to_mont(a.x, a.x);
        el_to_mont(a.y, a.y);
        // is_well_formed: y^2 = x^3 + a x + b (e.g. bls12_377_g1.cpp:367-385, mnt4_g2.cpp:430-452 with Z = 1)
        E y2, x3, b;
        el_sqr(y2, a.y);
        el_sqr(x3, a.x);
        el_mul(x3, x3, a.x);
        el_set_words(b, GP::COEFF_B);
        el_add(x3, x3, b);
        if constexpr (GP::COEFF_A != 0) {   // a lies in Fq (MNT4 G2: a' = 34 scales both components), as in the doublings
            E ax;
            el_mul_small<ec_coeff_a<E>::value>(ax, a.x);
            el_add(x3, x3, ax);
        }
        if (!el_eq(y2, x3)) bad |= 2u;
        else if (!in_safe_subgroup(a)) bad |= 4u;
    }
    if (bad) atomicOr(status, bad);
    store_aff(dst + i * AFFW, a);
}

__global__ void __launch_bounds__(TPB) k_ffi_decode_scalars(const uint32_t* __restrict__ src, size_t n,
                                                            uint32_t* __restrict__ dst, uint32_t* __restrict__ status) {
    const size_t i = gtid();
    if (i >= n) return;
    Fp<FR> s;
#pragma unroll
    for (int j = 0; j < FRW; ++j) s.v[j] = bswap32(src[i * FRW + FRW - 1 - j]);
    if (!fp_lt_modulus(s)) atomicOr(status, 1u);
    fp_store(dst + i * FRW, s);   // plain bigint: run the MSM with scalars_plain
}

// (x, y, 1) / (0, 1, 0) Montgomery record -> wire format (group_element_write, :173-187)
__global__ void k_ffi_encode_point(const uint32_t* __restrict__ src_xyz, uint32_t* __restrict__ dst) {
    if (gtid() != 0) return;
    E x, y;
    el_load(x, src_xyz);
    el_load(y, src_xyz + EW);
    el_from_mont(x, x);
    el_from_mont(y, y);
    store_coord_be(dst, x);
    store_coord_be(dst + EW, y);
}

// -------------------------------------------------------------- test hooks
__global__ void __launch_bounds__(TPB) k_field_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                  uint32_t* __restrict__ out, size_t n) {
    const size_t i = gtid();
    if (i >= n) return;
    E x, y, r;
    el_load(x, a + i * EW);
    if (b) el_load(y, b + i * EW); else el_zero(y);
    switch (op) {
    case 0: el_mul(r, x, y); break;
    case 1: el_sqr(r, x); break;
    case 2: el_add(r, x, y); break;
    case 3: el_sub(r, x, y); break;
    case 4: el_neg(r, x); break;
    case 5: el_inv(r, x); break;
    default: el_zero(r); break;
    }
    el_store(out + i * EW, r);
}

__global__ void __launch_bounds__(TPB) k_group_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                  uint32_t* __restrict__ out, size_t n, int form) {
    const size_t i = gtid();
    if (i >= n) return;
    Jac<E> p, q, r;
    load_libff(p, a + i * XYZW);
    if (op == 0) {
        load_libff(q, b + i * XYZW);
        jac_add(r, p, q);
    } else if (op == 1) {
        // second operand is in special form: Z == 1 or zero
        load_jac(q, b + i * XYZW);
        Aff<E> qa;
        if (el_is_zero(q.z)) {
            el_zero(qa.x);
            el_zero(qa.y);
        } else {
            qa.x = q.x;
            qa.y = q.y;
        }
        r = p;
        jac_madd(r, qa);
    } else {
        jac_dbl(r, p);
    }
    store_out(out + i * XYZW, r, form);
}

// Field-layer probe (group_vtable::field_probe): one lane per element, one library function per op code, on the
// element type T = E or EI.  The operands are taken as they are stored -- the almost-reduced ops get words in [0, 2p)
// per component -- and the result is stored as the function left it (no canonicalisation), so a test sees which
// representative came back.  Functions that exist per Fq component only run on each component of an Fq2 element.
template <class P, bool I, class F> AMDMSM_DEV void probe_comp1(Fp<P, I>& r, const Fp<P, I>& a, F f) { f(r, a); }
template <class P, int NR, bool I, class F> AMDMSM_DEV void probe_comp1(Fp2<P, NR, I>& r, const Fp2<P, NR, I>& a, F f) {
    f(r.c0, a.c0);
    f(r.c1, a.c1);
}
template <class P, bool I, class F> AMDMSM_DEV void probe_comp2(Fp<P, I>& r, const Fp<P, I>& a, const Fp<P, I>& b, F f) { f(r, a, b); }
template <class P, int NR, bool I, class F>
AMDMSM_DEV void probe_comp2(Fp2<P, NR, I>& r, const Fp2<P, NR, I>& a, const Fp2<P, NR, I>& b, F f) {
    f(r.c0, a.c0, b.c0);
    f(r.c1, a.c1, b.c1);
}
template <class T>
__global__ void __launch_bounds__(TPB) k_field_probe(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                     const uint32_t* __restrict__ c, const uint32_t* __restrict__ d,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ flag, size_t n) {
    using FC = Fp<FQ, std::is_same<T, EI>::value>;   // component type of T
    const size_t i = gtid();
    if (i >= n) return;
    T x, y, z, w, r;
    el_load(x, a + i * EW);
    if (b) el_load(y, b + i * EW); else el_zero(y);
    if (c) el_load(z, c + i * EW); else el_zero(z);
    if (d) el_load(w, d + i * EW); else el_zero(w);
    uint32_t f = 0;
    switch (op) {
    case FPROBE_MUL: el_mul(r, x, y); break;
    case FPROBE_SQR: el_sqr(r, x); break;
    case FPROBE_ADD: el_add(r, x, y); break;
    case FPROBE_SUB: el_sub(r, x, y); break;
    case FPROBE_NEG: el_neg(r, x); break;
    case FPROBE_INV: el_inv(r, x); break;
    case FPROBE_DBL: el_dbl(r, x); break;
    case FPROBE_CNEG: el_cneg(r, x, b && (b[i * EW] & 1u)); break;   // sense: low bit of b's first word
    case FPROBE_HALF: probe_comp1(r, x, [](FC& o, const FC& v) { fp_half(o, v); }); break;
    case FPROBE_TO_MONT: el_to_mont(r, x); break;
    case FPROBE_FROM_MONT: el_from_mont(r, x); break;
    case FPROBE_SQRT:
        el_zero(r);
        f = el_sqrt(r, x) ? 1u : 0u;
        break;
    case FPROBE_MUL_LZ: el_mul_lz(r, x, y); break;
    case FPROBE_SQR_LZ: el_sqr_lz(r, x); break;
    case FPROBE_SUB_LZ: el_sub_lz(r, x, y); break;
    case FPROBE_ADD_LZ: probe_comp2(r, x, y, [](FC& o, const FC& u, const FC& v) { fp_add_lz(o, u, v); }); break;
    case FPROBE_NEG_LZ: probe_comp1(r, x, [](FC& o, const FC& v) { fp_neg_lz(o, v); }); break;
    case FPROBE_MUL_SUB_MUL_LZ: el_mul_sub_mul_lz(r, x, y, z, w); break;
    case FPROBE_IS_ZERO_LZ:
        r = x;
        f = el_is_zero_lz(x) ? 1u : 0u;
        break;
    case FPROBE_CANON:
        r = x;
        el_canon(r);
        break;
    default: el_zero(r); break;
    }
    el_store(out + i * EW, r);
    if (flag) flag[i] = f;
}

// Point-level probe (group_vtable::xyzz_probe) of the extended-Jacobian functions of ec.cuh on T = E or EI.  acc: n
// (X, Y, ZZ, ZZZ) records of ZZW words taken as stored (xyzz_madd_lz: any representative in [0, 2p) per component); pt: n
// compact affine records (the mixed additions and xyzz_dbl_affine) or n more (X, Y, ZZ, ZZZ) records (xyzz_add); out: n
// records of ZZW words, stored as the function left them (xyzz_to_jac: X, Y, Z and ZZW - XYZW words of zero).
template <class T>
__global__ void __launch_bounds__(TPB) k_xyzz_probe(int op, const uint32_t* __restrict__ acc, const uint32_t* __restrict__ pt,
                                                    uint32_t* __restrict__ out, size_t n) {
    const size_t i = gtid();
    if (i >= n) return;
    Xyzz<T> a, r;
    Aff<T> p;
    load_xyzz(a, acc + i * ZZW);
    switch (op) {
    case XPROBE_MADD_LZ:
        load_aff(p, pt + i * AFFW);
        xyzz_madd_lz(a, p);
        r = a;
        break;
    case XPROBE_MADD:
        load_aff(p, pt + i * AFFW);
        xyzz_madd(a, p);
        r = a;
        break;
    case XPROBE_ADD: {
        Xyzz<T> q;
        load_xyzz(q, pt + i * ZZW);
        xyzz_add(r, a, q);
        break;
    }
    case XPROBE_DBL: xyzz_dbl(r, a); break;
    case XPROBE_DBL_AFFINE:
        load_aff(p, pt + i * AFFW);
        xyzz_dbl_affine(r, p);
        break;
    case XPROBE_TO_JAC: {
        Jac<T> j;
        xyzz_to_jac(j, a);
        r.x = j.x;
        r.y = j.y;
        r.zz = j.z;
        el_zero(r.zzz);
        break;
    }
    default: xyzz_set_inf(r); break;
    }
    store_xyzz(out + i * ZZW, r);
}

#if AMDMSM_ACC_RR
// Probes of the reduced-radix layer (rr.cuh; group_vtable::rr_probe / xyzz_rr_probe, tests/test_gpu_rr_probe.py).  Operands
// and results are RAW limbs: L int32 per Fq component, taken and stored as they are -- nothing is carried, reduced or
// range-checked on the way in or out, so a test chooses the representative and the spread over the limbs that a function
// meets and sees the ones it leaves.  One Fq component per lane: row t of every array belongs to lane t.  For the Fq2
// groups (ERR = Rr2H) element i is the lane pair (2 i, 2 i + 1) = (c0, c1); both lanes of a pair take the same branches
// and leave together, and flags are per pair.  No address depends on an operand's value.
constexpr int RRP_LANES = re_info<ERR>::PAIR ? 2 : 1;
// rr_first_reduced reads a table of 2^D + 1 multiples of p, which the library builds only where the first point needs the
// reduction (D = 5); the probe runs the function on every field whose table is as small (D <= 8: all but bw6_761, D = 16)
constexpr bool RRP_FIRST_REDUCED = rr_shape<FQ>::D <= 8;
AMDMSM_DEV void rrp_load(Rr<FQ>& r, const int32_t* q) {
#pragma unroll
    for (int i = 0; i < RRL; ++i) r.v[i] = q ? q[i] : 0;
}
AMDMSM_DEV void rrp_store(int32_t* q, const Rr<FQ>& r) {
#pragma unroll
    for (int i = 0; i < RRL; ++i) q[i] = r.v[i];
}
AMDMSM_DEV void rrp_load_words(uint32_t (&w)[FQ::N], const uint32_t* q) {
#pragma unroll
    for (int i = 0; i < FQ::N; ++i) w[i] = q ? q[i] : 0u;
}
AMDMSM_DEV void rrp_store_words(uint32_t* q, const uint32_t (&w)[FQ::N]) {
#pragma unroll
    for (int i = 0; i < FQ::N; ++i) q[i] = w[i];
}
// SET 0: the products (RRPROBE_MUL .. RRPROBE_EXPORT_D); SET 1: linear operations, conversions, constants and residue
// tests -- two kernels, so that no single one inlines every product of the widest field.
// a, b, c, d: n * RRP_LANES rows of L limbs (null: zeros); w: as many rows of N words (null: zeros); out: rows of L limbs;
// outw: rows of N words (zero where the op yields none); flag: one word per element.
template <int SET>
__global__ void __launch_bounds__(TPB) k_rr_probe(int op, int k, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                  const int32_t* __restrict__ c, const int32_t* __restrict__ d,
                                                  const uint32_t* __restrict__ w, int32_t* __restrict__ out,
                                                  uint32_t* __restrict__ outw, uint32_t* __restrict__ flag, size_t n) {
    constexpr int D = rr_shape<FQ>::D;
    constexpr int BL = rr_shape<FQ>::B * rr_shape<FQ>::L;
    const size_t t = gtid();
    const size_t i = t / RRP_LANES;
    if (i >= n) return;
    ERR x, y, z, u, r;
    rrp_load(re_comp(x), a ? a + t * RRL : nullptr);
    rrp_load(re_comp(y), b ? b + t * RRL : nullptr);
    rrp_load(re_comp(z), c ? c + t * RRL : nullptr);
    rrp_load(re_comp(u), d ? d + t * RRL : nullptr);
    uint32_t ww[FQ::N], ow[FQ::N];
    rrp_load_words(ww, w ? w + t * FQ::N : nullptr);
#pragma unroll
    for (int j = 0; j < FQ::N; ++j) ow[j] = 0;
    re_zero(r);
    bool f = false;
    if constexpr (SET == 0) {
        switch (op) {
        case RRPROBE_MUL: rr_mul(re_comp(r), re_comp(x), re_comp(y)); break;
        case RRPROBE_MUL2: rr_mul2(re_comp(r), re_comp(x), re_comp(y), re_comp(z), re_comp(u)); break;
        case RRPROBE_SQR: rr_sqr(re_comp(r), re_comp(x)); break;
        case RRPROBE_RE_MUL: re_mul(r, x, y); break;
        case RRPROBE_RE_SQR: re_sqr(r, x); break;
        case RRPROBE_RE_MUL_SUB_MUL: re_mul_sub_mul(r, x, y, z, u); break;
        case RRPROBE_MUL_POW2_32N: rr_mul_pow2<FQ, 32 * FQ::N>(re_comp(r), re_comp(x)); break;
        case RRPROBE_MUL_POW2_32N_D: rr_mul_pow2<FQ, 32 * FQ::N - D>(re_comp(r), re_comp(x)); break;
        case RRPROBE_FROM_WORDS_RHO: re_from_words_rho(r, ww); break;
        case RRPROBE_EXPORT_0:
            r = x;
            rr_export_component<FQ, 0>(ow, re_comp(x));
            break;
        case RRPROBE_EXPORT_D:
            r = x;
            rr_export_component<FQ, D>(ow, re_comp(x));
            break;
        default: break;
        }
    } else {
        switch (op) {
        case RRPROBE_NORM: rr_norm(re_comp(r), re_comp(x)); break;
        case RRPROBE_RIPPLE:
            r = x;
            rr_ripple(re_comp(r));
            break;
        case RRPROBE_SMALL_TIMES:
            if (k == 2) re_small_times(r, x, 2);
            else if (k == 3) re_small_times(r, x, 3);
            else re_small_times(r, x, 4);
            break;
        case RRPROBE_CNEG: rr_cneg(re_comp(r), re_comp(x), (i & 1u) != 0); break;   // negates the odd elements
        case RRPROBE_FROM_WORDS_0: rr_from_words<FQ, 0>(re_comp(r), ww); break;
        case RRPROBE_FROM_WORDS_D: rr_from_words<FQ, D>(re_comp(r), ww); break;
        case RRPROBE_FIRST_REDUCED:
            if constexpr (RRP_FIRST_REDUCED) rr_first_reduced<FQ>(re_comp(r), ww);
            break;
        case RRPROBE_FIRST_COORD: re_first_coord(r, ww); break;
        case RRPROBE_TO_WORDS:
            r = x;
            rr_to_words<FQ>(ow, re_comp(x));
            break;
        case RRPROBE_CANON_PRODUCT:
            r = x;
            rr_canon_product(re_comp(r));
            break;
        case RRPROBE_IS_ZERO_EXACT:
            r = x;
            f = re_is_zero_exact(x);
            break;
        case RRPROBE_MAYBE_ZERO_K:
            r = x;
            f = re_maybe_zero<rr_filter_k<FQ>()>(x);
            break;
        case RRPROBE_MAYBE_ZERO_64:
            r = x;
            f = re_maybe_zero<64>(x);
            break;
        case RRPROBE_SET_POW2_BL: re_set_pow2<BL>(r); break;
        case RRPROBE_SET_POW2_BL_D: re_set_pow2<BL + D>(r); break;
        default: break;
        }
    }
    rrp_store(out + t * RRL, re_comp(r));
    rrp_store_words(outw + t * FQ::N, ow);
    if (t % RRP_LANES == 0) flag[i] = f ? 1u : 0u;
}

// Point-level probe: one step of one point function of rr.cuh per element.  acc, sec, out: n * RRP_LANES rows of 4 L limbs
// (x, y, zz, zzz as a lane of k_accumulate holds them; the Jacobian ops read x, y, z from the first three and leave the
// fourth zero); pt: rows of 2 N words (this lane's component of an affine point); fin: one word per element -- bit 0 the
// accumulator is infinity, bit 1 the second operand is, bit 2 subtract (neg); fout: bit 0 the result is infinity, bit 1
// jac_is_inf_rr.  outw: rows of 4 N words, the result exported as the consumers of a record do it (rr_export_component on
// every coordinate: zz / zzz with the factor rho 2^D behind XRRPROBE_MADD / FIRST / EXPORT, rho behind every other op),
// zero for infinity.  SET 0: mixed addition, first point, conversions; SET 1: the general addition and doubling; SET 2:
// the Jacobian functions.
template <int SET>
__global__ void __launch_bounds__(TPB) k_xyzz_rr_probe(int op, const int32_t* __restrict__ acc, const int32_t* __restrict__ sec,
                                                       const uint32_t* __restrict__ pt, const uint32_t* __restrict__ fin,
                                                       int32_t* __restrict__ out, uint32_t* __restrict__ outw,
                                                       uint32_t* __restrict__ fout, size_t n) {
    constexpr int D = rr_shape<FQ>::D;
    const size_t t = gtid();
    const size_t i = t / RRP_LANES;
    if (i >= n) return;
    XyzzRr<ERR> p, q;
    const int32_t* pa = acc + t * 4 * RRL;
    rrp_load(re_comp(p.x), pa);
    rrp_load(re_comp(p.y), pa + RRL);
    rrp_load(re_comp(p.zz), pa + 2 * RRL);
    rrp_load(re_comp(p.zzz), pa + 3 * RRL);
    const int32_t* ps = sec ? sec + t * 4 * RRL : nullptr;
    rrp_load(re_comp(q.x), ps);
    rrp_load(re_comp(q.y), ps ? ps + RRL : nullptr);
    rrp_load(re_comp(q.zz), ps ? ps + 2 * RRL : nullptr);
    rrp_load(re_comp(q.zzz), ps ? ps + 3 * RRL : nullptr);
    uint32_t wx[FQ::N], wy[FQ::N];
    rrp_load_words(wx, pt ? pt + t * 2 * FQ::N : nullptr);
    rrp_load_words(wy, pt ? pt + t * 2 * FQ::N + FQ::N : nullptr);
    const uint32_t fi = fin ? fin[i] : 0u;
    bool inf = (fi & 1u) != 0;
    const bool q_inf = (fi & 2u) != 0, neg = (fi & 4u) != 0;
    bool is_inf = false;
    bool rho = true;   // zz / zzz of the result carry the factor rho (else rho 2^D)
    if constexpr (SET == 0) {
        switch (op) {
        case XRRPROBE_MADD:
            xyzz_madd_rr(p, inf, wx, wy, neg);
            rho = false;
            break;
        case XRRPROBE_FIRST:
            xyzz_rr_first(p, wx, wy, neg);
            inf = false;
            rho = false;
            break;
        case XRRPROBE_REC_TO_RHO: xyzz_rec_to_rho(p); break;
        case XRRPROBE_EXPORT: rho = false; break;
        default: break;
        }
    } else if constexpr (SET == 1) {
        switch (op) {
        case XRRPROBE_DBL_RHO: xyzz_dbl_rho(p, inf); break;
        case XRRPROBE_ADD_RHO: xyzz_add_rho(p, inf, q, q_inf); break;
        default: break;
        }
    } else {
        JacRr<ERR> j;
        j.x = p.x;
        j.y = p.y;
        j.z = p.zz;
        switch (op) {
        case XRRPROBE_JAC_DBL: jac_dbl_rr(j, inf); break;
        case XRRPROBE_JAC_MADD: jac_madd_rr(j, inf, q.x, q.y); break;
        case XRRPROBE_JAC_IS_INF: is_inf = jac_is_inf_rr(j, inf); break;
        default: break;
        }
        p.x = j.x;
        p.y = j.y;
        p.zz = j.z;
        re_zero(p.zzz);
    }
    int32_t* po = out + t * 4 * RRL;
    rrp_store(po, re_comp(p.x));
    rrp_store(po + RRL, re_comp(p.y));
    rrp_store(po + 2 * RRL, re_comp(p.zz));
    rrp_store(po + 3 * RRL, re_comp(p.zzz));
    uint32_t ow[4][FQ::N];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < FQ::N; ++j) ow[c][j] = 0;
    if (!inf) {
        rr_export_component<FQ, 0>(ow[0], re_comp(p.x));
        rr_export_component<FQ, 0>(ow[1], re_comp(p.y));
        if (rho) {
            rr_export_component<FQ, 0>(ow[2], re_comp(p.zz));
            rr_export_component<FQ, 0>(ow[3], re_comp(p.zzz));
        } else {
            rr_export_component<FQ, D>(ow[2], re_comp(p.zz));
            rr_export_component<FQ, D>(ow[3], re_comp(p.zzz));
        }
    }
    uint32_t* pw = outw + t * 4 * FQ::N;
#pragma unroll
    for (int c = 0; c < 4; ++c) rrp_store_words(pw + c * FQ::N, ow[c]);
    if (t % RRP_LANES == 0) fout[i] = (inf ? 1u : 0u) | (is_inf ? 2u : 0u);
}
#endif

// Throughput probes: a dependent chain of Montgomery products / mixed additions per lane,
// operands in registers, no memory traffic inside the loop.
template <bool I>
__global__ void __launch_bounds__(TPB) k_mul_bench(uint32_t* __restrict__ inout, size_t nthreads, int iters) {
    const size_t i = gtid();
    if (i >= nthreads) return;
    Fp<FQ, I> x, y;
    fp_load(x, inout + i * FQ::N);
    y = x;
    for (int k = 0; k < iters; ++k) {
        fp_mul(x, x, y);
        fp_mul(y, y, x);
    }
    fp_add(x, x, y);
    fp_store(inout + i * FQ::N, x);
}

template <class T>
__global__ void __launch_bounds__(TPB) k_xyzz_madd_bench(const uint32_t* __restrict__ pts, uint32_t* __restrict__ out,
                                                         size_t nthreads, int iters) {
    const size_t i = gtid();
    if (i >= nthreads) return;
    Aff<T> p;
    load_aff(p, pts + i * AFFW);
    Xyzz<T> acc;
    xyzz_dbl_affine(acc, p);
    for (int k = 0; k < iters; ++k) xyzz_madd(acc, p);
    Jac<T> j;
    xyzz_to_jac(j, acc);
    store_jac(out + i * XYZW, j);
}

template <class T>
__global__ void __launch_bounds__(TPB) k_madd_bench(const uint32_t* __restrict__ pts, uint32_t* __restrict__ out,
                                                    size_t nthreads, int iters) {
    const size_t i = gtid();
    if (i >= nthreads) return;
    Aff<T> p;
    load_aff(p, pts + i * AFFW);
    Jac<T> acc;
    jac_from_aff(acc, p);
    jac_dbl(acc, acc);
    for (int k = 0; k < iters; ++k) jac_madd(acc, p);
    store_jac(out + i * XYZW, acc);
}

#if AMDMSM_ACC_RR
// The same on reduced-radix limbs (rr.cuh) for the groups with coordinates in Fq: one loop over the windows (the
// scalar is shifted down window by window, so the mixed addition is emitted once), the accumulator exported to
// canonical words at the end -- in uniform control flow, once per lane.  window < 32.
template <class G>   // G = GP; a template only so that the Fq2 groups do not instantiate it
__global__ void __launch_bounds__(TPB, 2) k_fb_exp_rr(const uint32_t* __restrict__ table_aff, const uint32_t* __restrict__ scalars,
                                                      size_t n, int mont, const uint32_t* __restrict__ coeff, int scalar_size,
                                                      int window, int form, uint32_t* __restrict__ out) {
    static_assert(G::DEG == 1, "prime-field groups");
    using FQ = typename G::fq;
    using E = Fp<FQ, (AMDMSM_COLD_INLINE != 0)>;
    const size_t i = gtid();
    if (i >= n) return;
    Fp<FR> x;
    fp_load(x, scalars + i * FRW);
    if (coeff) {   // coeff * v[i] (batch_exp_with_coeff, multiexp.tcc:937)
        Fp<FR> cf;
        fp_load(cf, coeff);
        if (!mont) {
            fp_to_mont(x, x);
            fp_to_mont(cf, cf);
        }
        fp_mul(x, x, cf);
        fp_from_mont(x, x);
    } else if (mont) {
        fp_from_mont(x, x);
    }
    const int outerc = (scalar_size + window - 1) / window;
    const size_t row_len = (size_t)1 << window;
    const uint32_t wmask = (1u << window) - 1u;
    XyzzRr<Rr<FQ>> acc;
    rr_zero(acc.x); rr_zero(acc.y); rr_zero(acc.zz); rr_zero(acc.zzz);
    bool inf = true;   // powers_of_g[0][0] = zero
    aff_words e;
    // the entry of window `outer` (digit 0 names the zero entry: an all-zero record is skipped by the addition as an
    // infinite point); the scalar is shifted down as its digits are taken
    auto fetch = [&](int outer) {
        const uint32_t inner = x.v[0] & wmask;
#pragma unroll
        for (int j = 0; j < FRW; ++j) x.v[j] = __builtin_amdgcn_alignbit(j + 1 < FRW ? x.v[j + 1] : 0u, x.v[j], (uint32_t)window);
#pragma unroll
        for (int j = 0; j < FQ::N; ++j) e.x[j] = e.y[j] = 0;
        if (inner) aff_words_load(e, table_aff + ((size_t)outer * row_len + inner) * AFFW);
    };
    fetch(0);
    for (int outer = 0; outer < outerc; ++outer) {
        // the next entry travels under the second half of this addition (xyzz_madd_rr's mid hook)
        xyzz_madd_rr(acc, inf, e.x, e.y, false, [&] {
            if (outer + 1 < outerc) fetch(outer + 1);
        });
    }
    constexpr int D = rr_shape<FQ>::D;
    Xyzz<E> a;
    if (inf) {
        xyzz_set_inf(a);
    } else {
        rr_export_component<FQ, 0>(a.x.v, acc.x);
        rr_export_component<FQ, 0>(a.y.v, acc.y);
        rr_export_component<FQ, D>(a.zz.v, acc.zz);
        rr_export_component<FQ, D>(a.zzz.v, acc.zzz);
    }
    Jac<E> res;
    xyzz_to_jac(res, a);
    store_out(out + i * XYZW, res, form);
}
#endif

// ---------------------------------------------------------------- element-wise scalar multiplication
// out[i] = k_i * P_i, one lane per element (amdmsm_scalar_mul_vec): a signed fixed-window ladder over a table of the
// lane's own small multiples.  Entry j of element i, the affine point (j + 1) P_i, is record j * n + i of the table, so
// that the lanes of a wave, which read one entry index each at the same step of the ladder, read neighbouring records
// whenever their digits agree in magnitude.
constexpr int SMV_W = 4;                      // window width
constexpr int SMV_T = 1 << (SMV_W - 1);       // table entries per element: 1 P .. 2^(w-1) P
constexpr int SMV_DIGITS = (32 * FRW + SMV_W - 1) / SMV_W + 1;   // the last digit is the carry out of the top window
static_assert(32 % SMV_W == 0, "the digits are packed whole into 32-bit words");
// A scalar's digits as a row of signed bytes (segmented MSM, fold): bytes between two rows, whole words
constexpr int SMV_DS = (SMV_DIGITS + 3) / 4 * 4;
// row[w] = digit w of W, as the calls of for_each_signed_digit hand them over: `word` gathers four of them and goes out
// behind the fourth, or behind the last
AMDMSM_DEV void put_digit_byte(uint32_t* row, uint32_t& word, int w, int W, int32_t d) {
    word |= ((uint32_t)d & 0xffu) << ((w & 3) * 8);
    if ((w & 3) == 3 || w == W - 1) {
        row[w >> 2] = word;
        word = 0;
    }
}

// table[j * n + i] = (j + 1) P_i, affine.  The multiples are built in Jacobian coordinates by repeated mixed addition of
// P_i (the first addition copies P_i, the second meets the equal point and doubles) and made affine with one inversion per
// lane, Montgomery's trick over the lane's own entries as in k_fb_table_affine: tmp[j * n + i] holds Z_j and the product
// of the Z's before it between the two passes.  An infinite multiple (P_i infinite, or of order <= 2^(w-1)) becomes (0, 0).
__global__ void __launch_bounds__(TPB) k_smv_table(const uint32_t* __restrict__ bases, size_t n, uint32_t* __restrict__ tmp,
                                                   uint32_t* __restrict__ table) {
    const size_t i = gtid();
    if (i >= n) return;
    Aff<E> p;
    load_aff(p, bases + i * AFFW);
    Jac<E> q;
    jac_set_inf(q);
    E acc;
    el_one(acc);
#pragma unroll 1
    for (int j = 0; j < SMV_T; ++j) {
        jac_madd(q, p);
        const size_t rec = ((size_t)j * n + i) * AFFW;
        el_store(table + rec, q.x);
        el_store(table + rec + EW, q.y);
        el_store(tmp + rec, q.z);
        el_store(tmp + rec + EW, acc);   // prefix product of the Z's before this entry
        if (!jac_is_inf(q)) el_mul(acc, acc, q.z);
    }
    E inv;
    el_inv(inv, acc);
#pragma unroll 1
    for (int j = SMV_T; j-- > 0;) {
        const size_t rec = ((size_t)j * n + i) * AFFW;
        E z;
        el_load(z, tmp + rec);
        Aff<E> a;
        if (el_is_zero(z)) {
            el_zero(a.x);
            el_zero(a.y);
        } else {
            E pre, zi, z2;
            el_load(pre, tmp + rec + EW);
            load_aff(a, table + rec);
            el_mul(zi, inv, pre);      // Z_j^-1
            el_mul(inv, inv, z);
            el_sqr(z2, zi);
            el_mul(a.x, a.x, z2);
            el_mul(z2, z2, zi);
            el_mul(a.y, a.y, z2);
        }
        store_aff(table + rec, a);
    }
}

// The ladder: the scalar recoded to signed radix-2^w digits (for_each_signed_digit, one digit more than the scalar's
// words hold for the carry out of the top window, so a plain scalar may be any integer of 32 FRW bits), taken from the
// top: w doublings of the XYZZ accumulator, then the mixed addition of +-table[|d| - 1] -- xyzz_madd, whose equal-point
// branch doubles with the a != 0 term and whose opposite-point branch gives infinity.  A digit lies in [-2^(w-1),
// 2^(w-1)), so it is kept as a w-bit two's-complement field; the packed digits are shifted up window by window and no
// private array is indexed at run time.  acc, infinity on entry, becomes s * P_i, P_i being element i of the n the table
// holds; e is the caller's record for the table's entries.
AMDMSM_DEV void smv_ladder_run(Xyzz<E>& acc, Aff<E>& e, const uint32_t* __restrict__ table, size_t n, size_t i,
                               const uint32_t (&s)[FRW]) {
    constexpr int PER = 32 / SMV_W;
    constexpr uint32_t DMASK = (1u << SMV_W) - 1u;
    uint32_t rec[FRW];
    uint32_t top = 0;
#pragma unroll
    for (int j = 0; j < FRW; ++j) rec[j] = 0;
    for_each_signed_digit(s, SMV_W, SMV_DIGITS, [&](int w, int32_t d) {
        const uint32_t f = ((uint32_t)d & DMASK) << ((w % PER) * SMV_W);
#pragma unroll
        for (int j = 0; j < FRW; ++j) rec[j] |= (w / PER == j) ? f : 0u;
        top |= (w / PER == FRW) ? f : 0u;
    });
    // the carry digit is 0 or 1
    if (top) {
        load_aff(e, table + i * AFFW);
        xyzz_madd(acc, e);
    }
#pragma unroll 1
    for (int w = SMV_DIGITS - 2; w >= 0; --w) {
#pragma unroll 1
        for (int k = 0; k < SMV_W; ++k) xyzz_dbl(acc, acc);
        const uint32_t f = rec[FRW - 1] >> (32 - SMV_W);
#pragma unroll
        for (int j = FRW - 1; j >= 0; --j) rec[j] = (rec[j] << SMV_W) | (j ? rec[j - 1] >> (32 - SMV_W) : 0u);
        const bool neg = (f >> (SMV_W - 1)) != 0;
        const uint32_t mag = neg ? (1u << SMV_W) - f : f;
        if (mag) {
            load_aff(e, table + ((size_t)(mag - 1) * n + i) * AFFW);
            el_cneg(e.y, e.y, neg);
            xyzz_madd(acc, e);
        }
    }
}

__global__ void __launch_bounds__(TPB) k_smv_ladder(const uint32_t* __restrict__ table, size_t n,
                                                    const uint32_t* __restrict__ scalars, int mont, int form,
                                                    uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    uint32_t s[FRW];
    load_scalar(s, scalars, i, mont);
    Xyzz<E> acc;
    xyzz_set_inf(acc);
    Aff<E> e;
    smv_ladder_run(acc, e, table, n, i, s);
    Jac<E> res;
    xyzz_to_jac(res, acc);
    store_out(out + i * XYZW, res, form);
}

// ---------------------------------------------------------------- segmented MSM
// out[j] = sum of k_t * P_t over the terms of segment j, many short segments in one pass (amdmsm_multi_exp_segments).
// The terms share the ladder's table (k_smv_table) and its signed 4-bit digits, but a lane owns one (slice, window)
// pair instead of one term: it adds +-table[|d| - 1] of every term of its slice -- a slice is a segment, or a piece of
// a long one -- and no lane doubles anything.  The doublings are paid once per segment, in the Horner chain over its
// SMV_DIGITS window sums.

// digits[t * SMV_DS + w] = digit w of scalar t as a signed byte: the lanes of one segment, which step through its terms
// together and differ only in w, read one term's digits from neighbouring bytes.  One pass of its own: recoding inside
// the accumulation lane would repeat the scalar's Montgomery reduction SMV_DIGITS times per term.
__global__ void __launch_bounds__(TPB) k_seg_digits(const uint32_t* __restrict__ scalars, size_t n, int mont,
                                                    uint32_t* __restrict__ digits) {
    const size_t i = gtid();
    if (i >= n) return;
    uint32_t s[FRW];
    load_scalar(s, scalars, i, mont);
    uint32_t* row = digits + i * (SMV_DS / 4);
    uint32_t word = 0;
    for_each_signed_digit(s, SMV_W, SMV_DIGITS, [&](int w, int32_t d) { put_digit_byte(row, word, w, SMV_DIGITS, d); });
}

// Lane L = slice * SMV_DIGITS + w.  slices[s] = (first term, end term, table column of the first term, -): terms count
// from the start of `digits`, columns index the table's rows of nt records (the term itself, or with shared bases its
// place in the segment).  A wave lies inside one slice except where two meet (SMV_DIGITS is 65, 81 or 97), so its lanes
// run the same number of steps wherever neighbouring slices are equally long.  The addition is the complete xyzz_madd;
// a zero digit is skipped.  sums[L] = the lane's window sum, (X, Y, ZZ, ZZZ).
__global__ void __launch_bounds__(TPB) k_seg_accumulate(const uint32_t* __restrict__ table, size_t nt,
                                                        const signed char* __restrict__ digits,
                                                        const uint4* __restrict__ slices, size_t lanes,
                                                        uint32_t* __restrict__ sums) {
    const size_t lane = gtid();
    if (lane >= lanes) return;
    const size_t sl = lane / SMV_DIGITS;
    const uint32_t w = (uint32_t)(lane - sl * SMV_DIGITS);
    const uint4 s = slices[sl];
    Xyzz<E> acc;
    xyzz_set_inf(acc);
    Aff<E> e;
    const signed char* dp = digits + (size_t)s.x * SMV_DS + w;
    size_t col = s.z;
#pragma unroll 1
    for (uint32_t t = s.x; t < s.y; ++t, ++col, dp += SMV_DS) {
        const int d = *dp;
        if (d) {
            const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            load_aff(e, table + ((size_t)(mag - 1) * nt + col) * AFFW);
            el_cneg(e.y, e.y, d < 0);
            xyzz_madd(acc, e);
        }
    }
    store_xyzz(sums + lane * ZZW, acc);
}

// winsum[seg * SMV_DIGITS + w] = sum over the segment's slices [seg_first[seg], seg_first[seg + 1]) of their window
// sum w, as an engine-Jacobian record for the Horner chain; a segment without slices (an empty one) gives infinity
__global__ void __launch_bounds__(TPB) k_seg_fold(const uint32_t* __restrict__ sums, const uint32_t* __restrict__ seg_first,
                                                  size_t lanes, uint32_t* __restrict__ winsum) {
    const size_t lane = gtid();
    if (lane >= lanes) return;
    const size_t seg = lane / SMV_DIGITS;
    const uint32_t w = (uint32_t)(lane - seg * SMV_DIGITS);
    Xyzz<E> acc, x;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (uint32_t sl = seg_first[seg]; sl < seg_first[seg + 1]; ++sl) {
        load_xyzz(x, sums + ((size_t)sl * SMV_DIGITS + w) * ZZW);
        xyzz_add(acc, acc, x);
    }
    Jac<E> r;
    xyzz_to_jac(r, acc);
    store_jac(winsum + lane * XYZW, r);
}

// one wave per segment: the Horner chain of k_horner over the segment's window sums, SMV_W doublings between them
__global__ void __launch_bounds__(64) k_seg_horner(const uint32_t* __restrict__ winsum, int form, uint32_t* __restrict__ out) {
    Jac<E> res;
    horner_chain(res, winsum + (size_t)blockIdx.x * SMV_DIGITS * XYZW, SMV_DIGITS, SMV_W, nullptr);
    if (threadIdx.x == 0) store_out(out + (size_t)blockIdx.x * XYZW, res, form);
}
template <class EE = E>
__global__ void __launch_bounds__(64) k_seg_horner_lazy(const uint32_t* __restrict__ winsum, int form, uint32_t* __restrict__ out) {
    Jac<EE> res;
    horner_chain_lazy(res, winsum + (size_t)blockIdx.x * SMV_DIGITS * XYZW, SMV_DIGITS, SMV_W, nullptr);
    if (threadIdx.x == 0) store_out(out + (size_t)blockIdx.x * XYZW, res, form);
}

// Launches of the Horner kernels: the lazy chain where the group has one and AMDMSM_HORNER_LAZY does not say 0.  The
// kernel's element type hangs on OK so that the other groups never instantiate the lazy kernels.
template <bool OK> struct horner_lazy_el { using type = E; };
template <bool OK = HORNER_LAZY_OK>
void launch_horner(hipStream_t st, const uint32_t* window_sums, int W, int c, int form, const uint32_t* init, uint32_t* out) {
    if constexpr (OK) {
        if (horner_lazy()) {
            hipLaunchKernelGGL(k_horner_lazy<typename horner_lazy_el<OK>::type>, dim3(1), dim3(64), 0, st, window_sums, W, c, form, init, out);
            return;
        }
    }
    hipLaunchKernelGGL(k_horner, dim3(1), dim3(64), 0, st, window_sums, W, c, form, init, out);
}
template <bool OK = HORNER_LAZY_OK>
void launch_horner_batch(hipStream_t st, const uint32_t* window_sums, int k, int W, int c, int form, const horner_outs& o) {
    if constexpr (OK) {
        if (horner_lazy()) {
            hipLaunchKernelGGL(k_horner_batch_lazy<typename horner_lazy_el<OK>::type>, dim3((unsigned)k), dim3(64), 0, st, window_sums, W, c, form, o);
            return;
        }
    }
    hipLaunchKernelGGL(k_horner_batch, dim3((unsigned)k), dim3(64), 0, st, window_sums, W, c, form, o);
}
template <bool OK = HORNER_LAZY_OK>
void launch_window_horner(hipStream_t st, const uint32_t* planes, int W, int c, uint32_t* out) {
    const dim3 threads((unsigned)(64 * ((c + 3) / 4)));
    if constexpr (OK) {
        if (horner_lazy()) {
            hipLaunchKernelGGL(k_window_horner_lazy<typename horner_lazy_el<OK>::type>, dim3((unsigned)W), threads, 0, st, planes, c, out);
            return;
        }
    }
    hipLaunchKernelGGL(k_window_horner, dim3((unsigned)W), threads, 0, st, planes, c, out);
}
template <bool OK = HORNER_LAZY_OK>
void launch_seg_horner(hipStream_t st, const uint32_t* winsum, size_t m, int form, uint32_t* out) {
    if constexpr (OK) {
        if (horner_lazy()) {
            hipLaunchKernelGGL(k_seg_horner_lazy<typename horner_lazy_el<OK>::type>, dim3((unsigned)m), dim3(64), 0, st, winsum, form, out);
            return;
        }
    }
    hipLaunchKernelGGL(k_seg_horner, dim3((unsigned)m), dim3(64), 0, st, winsum, form, out);
}

// ---------------------------------------------------------------- fold of point vectors by shared scalars
// out[i] = s_0 P_0[i] + ... + s_(k-1) P_(k-1)[i], one lane per element (amdmsm_fold_vec).  The k scalars are the same
// for every element, so the digits are uniform over the grid: one doubling chain serves all rows (Straus), windows
// above the highest nonzero digit are skipped by everybody, and no branch on a digit diverges.  Every P_j has the
// ladder's table (k_smv_table); with the endomorphism split each scalar gives two half-length rows, and the row of
// phi(P_j) reads P_j's table with x scaled by beta.
static_assert(2 * FOLD_MAX_K * SMV_DS <= (int)FOLD_DIGIT_BYTES, "the digit rows fit the buffer the engine sets aside");
struct alignas(16) fold_scalars {
    uint32_t w[FOLD_MAX_K * FRW];
};

// One lane per scalar.  digits[row * SMV_DS + w] = digit w of the row as a signed byte, whole words written: without
// the split row j holds the SMV_DIGITS digits of scalar j (the carry digit included), with it rows 2 j and 2 j + 1
// hold the W digits of its halves, which belong to P_j and phi(P_j).
__global__ void __launch_bounds__(64) k_fold_digits(const fold_scalars sc, int k, int mont, int glv, int W,
                                                    uint32_t* __restrict__ digits) {
    const int j = (int)threadIdx.x;
    if (j >= k) return;
    uint32_t s[FRW];
    load_scalar(s, sc.w, (size_t)j, mont);
    uint32_t word = 0;
    auto put = [&](int row, int w, int32_t d) { put_digit_byte(digits + row * (SMV_DS / 4), word, w, W, d); };
    if (glv) {
        if constexpr (GP::HAS_ENDO) for_each_glv_digit(s, SMV_W, W, [&](int h, int w, int32_t d) { put(2 * j + h, w, d); });
    } else {
        for_each_signed_digit(s, SMV_W, W, [&](int w, int32_t d) { put(j, w, d); });
    }
}

// The ladder.  The digit buffer is read through addresses that depend on nothing but the kernel's arguments and the
// loop counters: first a scan, four windows at a time, for the highest window in which some row has a nonzero digit
// (none: n infinities, no table is read), then from there down SMV_W doublings per window and, for every row with a
// nonzero digit d, the mixed addition of +-table_j[|d| - 1] -- the complete xyzz_madd, as in k_smv_ladder.
__global__ void __launch_bounds__(TPB) k_fold_ladder(const uint32_t* __restrict__ tables, size_t n,
                                                     const uint32_t* __restrict__ digits, int rows, int glv, int W,
                                                     int form, uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n) return;
    int top = -1;
#pragma unroll 1
    for (int q = (W + 3) / 4 - 1; q >= 0 && top < 0; --q) {
        uint32_t any = 0;   // a byte of it is nonzero where some row has a nonzero digit in window 4 q + byte
#pragma unroll 1
        for (int r = 0; r < rows; ++r) any |= digits[r * (SMV_DS / 4) + q];
        if (any) top = 4 * q + (31 - __clz((int)any)) / 8;
    }
    const signed char* dg = (const signed char*)digits;
    Xyzz<E> acc;
    xyzz_set_inf(acc);
    Aff<E> e;
#pragma unroll 1
    for (int w = top; w >= 0; --w) {
        if (w != top) {
#pragma unroll 1
            for (int b = 0; b < SMV_W; ++b) xyzz_dbl(acc, acc);
        }
#pragma unroll 1
        for (int r = 0; r < rows; ++r) {
            const int d = dg[r * SMV_DS + w];
            if (d) {
                const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
                const size_t t = (size_t)(glv ? r >> 1 : r);
                load_aff(e, tables + ((t * SMV_T + (mag - 1)) * n + i) * AFFW);
                if constexpr (GP::HAS_ENDO) {
                    if (glv && (r & 1)) scale_by_beta(e.x);   // phi(x, y) = (beta x, y); (0, 0) stays infinity
                }
                el_cneg(e.y, e.y, d < 0);
                xyzz_madd(acc, e);
            }
        }
    }
    Jac<E> res;
    xyzz_to_jac(res, acc);
    store_out(out + i * XYZW, res, form);
}

// ---------------------------------------------------------------- radix-2 FFT over a point vector
// out[j] = sum_i w^(i j) P_i (amdmsm_group_fft), n = 2^L, as L autosorting decimation-in-time stages.  Before stage t
// (h = 2^t, r = n / 2^t) record q + r k of the vector is value k of the length-h transform of the r-strided subsequence
// that starts at q; the stage joins the subsequences q and q + r / 2.  With r2 = r / 2, butterfly b = q + r2 k of the
// n / 2 (q < r2, k < h) reads
//     A = in[q + r k] = in[b + (b & ~(r2 - 1))],   B = in[that + r2],   w = twiddles[k r2] = twiddles[b & ~(r2 - 1)]
// and writes A + w B to record b and A - w B to record b + n / 2, so stage L - 1 leaves natural order and no index is
// bit-reversed.  Stage 0 has k = 0 alone -- every twiddle is 1 -- and runs without table and ladder.  No index depends
// on a twiddle's value.
AMDMSM_DEV size_t fft_a_index(size_t b, int rsh) { return b + ((b >> rsh) << rsh); }   // rsh = log2 r2

// dst[i] = the B operand of butterfly b0 + i, i < cn: the contiguous base vector k_smv_table wants.  One lane per 16 bytes.
__global__ void __launch_bounds__(TPB) k_fft_gather(const uint32_t* __restrict__ in, size_t b0, size_t cn, int rsh,
                                                    uint32_t* __restrict__ dst) {
    constexpr size_t PARTS = AFFW / 4;
    static_assert(AFFW % 4 == 0, "a compact affine record is a whole number of 16-byte parts");
    const size_t t = gtid();
    if (t >= cn * PARTS) return;
    const size_t i = t / PARTS, part = t % PARTS;
    const size_t ib = fft_a_index(b0 + i, rsh) + ((size_t)1 << rsh);
    reinterpret_cast<uint4*>(dst)[t] = reinterpret_cast<const uint4*>(in + ib * AFFW)[part];
}

// One lane per butterfly b0 + i.  LADDER: T = w B by smv_ladder_run over the table of the chunk's B operands; else
// T = B.  Only then A is loaded, and both results go through the complete mixed addition: T + A, and A - T as
// -(T + (-A)).  Infinite A or T, A = T (xyzz_madd doubles, with the a != 0 term) and A = -T take xyzz_madd's own
// branches.  out: libff records b and b + half of the stage's result vector.
template <bool LADDER>
__global__ void __launch_bounds__(TPB) k_fft_butterfly(const uint32_t* __restrict__ table, size_t cn,
                                                       const uint32_t* __restrict__ in, size_t b0, int rsh,
                                                       const uint32_t* __restrict__ twiddles, int mont, size_t half,
                                                       uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= cn) return;
    const size_t b = b0 + i, ia = fft_a_index(b, rsh);
    Xyzz<E> acc;
    xyzz_set_inf(acc);
    Aff<E> e;
    if constexpr (LADDER) {
        uint32_t s[FRW];
        load_scalar(s, twiddles, (b >> rsh) << rsh, mont);
        smv_ladder_run(acc, e, table, cn, i, s);
    } else {
        load_aff(e, in + (ia + ((size_t)1 << rsh)) * AFFW);
        xyzz_madd(acc, e);
    }
    load_aff(e, in + ia * AFFW);
    Xyzz<E> dif = acc;
    Jac<E> res;
    xyzz_madd(acc, e);
    xyzz_to_jac(res, acc);
    store_out(out + b * XYZW, res, OUT_LIBFF);
    el_cneg(e.y, e.y, true);
    xyzz_madd(dif, e);
    el_cneg(dif.y, dif.y, true);
    xyzz_to_jac(res, dif);
    store_out(out + (b + half) * XYZW, res, OUT_LIBFF);
}

// ---------------------------------------------------------------- launchers
inline unsigned blocks_for(size_t n, int tpb = TPB) { return (unsigned)((n + tpb - 1) / tpb); }

void l_import_bases(hipStream_t st, const uint32_t* src, size_t stride_words, int form_special, size_t n, uint32_t* dst) {
    if (!n) return;
    const size_t lanes = form_special ? n : (n + IMPORT_K - 1) / IMPORT_K;
    hipLaunchKernelGGL(k_import_bases, dim3(blocks_for(lanes)), dim3(TPB), 0, st, src, stride_words, form_special, n, dst);
}
void l_precompute_table(hipStream_t st, const uint32_t* bases, size_t n, int c, int D, uint32_t* tmp, uint32_t* table) {
    if (!n) return;
    hipLaunchKernelGGL(k_precompute_table, dim3(blocks_for(n)), dim3(TPB), 0, st, bases, n, c, D, tmp, table);
}
void l_count(hipStream_t st, const uint32_t* scalars, size_t n, int mont, int c, int W, uint32_t* counts) {
    if (!n) return;
    hipLaunchKernelGGL(k_count, dim3(blocks_for(n)), dim3(TPB), 0, st, scalars, n, mont, c, W, counts);
    hipLaunchKernelGGL(k_scan, dim3(W), dim3(SCAN_TPB), 0, st, counts, (uint32_t)1 << (c - 1));
}
void l_scalar_stats(hipStream_t st, const uint32_t* scalars, size_t n, int mont, uint32_t* stats) {
    if (!n) return;
    const unsigned blocks = (unsigned)std::min<size_t>((n + TPB - 1) / TPB, 4096);
    hipLaunchKernelGGL(k_scalar_stats, dim3(blocks), dim3(TPB), 0, st, scalars, n, mont, stats);
}
void l_scatter(hipStream_t st, const uint32_t* scalars, size_t n, int mont, int c, int W, uint32_t* cursor,
               uint32_t* lists, size_t list_stride) {
    if (!n) return;
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for(n)), dim3(TPB), 0, st, scalars, n, mont, c, W, cursor, lists, list_stride);
}
template <int WB>
size_t packed_items(const void* p, size_t n) { return packed_split<WB>(p, n).items(); }
// group_vtable::sort_top_window; flat lists have one window
int l_sort_top_window(int mode, int mont, int c, int W, size_t columns, int* tb_out) {
    const bool flat = mode == 1;
    const int tb = flat ? c - 1 : top_window_bits(mode == 2 ? GLV::BOUND_LOG2_X1000 : 0, mont ? FR::BITS : 32 * FRW, c, W);
    if (tb_out) *tb_out = tb;
    return flat ? 0 : sort_top_shift(tb, c, W, sort_geometry(columns, c, W).fb);
}
// Workgroups of a digit-pass kernel the current device holds at once with `lds` bytes of dynamic LDS: resident workgroups
// per CU times CUs, asked once per (thread, device, kernel, LDS size) and remembered -- consecutive calls of a context
// repeat the same question.  AMDMSM_SORT_DIGIT_WGS overrides.
uint32_t digit_pass_workgroups(const void* kernel, size_t lds) {
    // AMDMSM_SORT_DIGIT_WGS=k: the digit pass on k workgroups (tests, sweeps); 0 / unset: what the device holds at once
    static const int forced = getenv("AMDMSM_SORT_DIGIT_WGS") ? atoi(getenv("AMDMSM_SORT_DIGIT_WGS")) : 0;
    if (forced > 0) return (uint32_t)forced;
    struct answer {
        int dev;
        const void* kernel;
        size_t lds;
        uint32_t wgs;
    };
    // seven digit kernels (k_sort_digits, _sel, _short<0, 1, 2, 4, 8>), each with the LDS sizes of the plans in use
    constexpr unsigned MEMO = 32;
    thread_local answer memo[MEMO] = {};
    thread_local unsigned next = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (const answer& a : memo)
        if (a.wgs && a.dev == dev && a.kernel == kernel && a.lds == lds) return a.wgs;
    int cus = 0, per_cu = 0;
    // a query that fails is not remembered and not replaced by a guess: 0 = unknown, the grid rule's fallback
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0 ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SORT_TPB, lds) != hipSuccess || per_cu <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    answer& a = memo[next++ % MEMO];
    a = answer{dev, kernel, lds, (uint32_t)cus * (uint32_t)per_cu};
    return a.wgs;
}
// group_vtable::sort.  The form of src picks the digit pass; everything behind it is the same
void l_sort(hipStream_t st, const sort_src& src, size_t n, int mont, int c, int W, const sort_bufs& b, int mode) {
    if (!n) return;
    const uint32_t* scalars = (const uint32_t*)src.scalars;
    const sort_src::short_form* ss = src.form == sort_src::SHORT ? &src.shrt : nullptr;
    const scalar_sel* sel = src.form == sort_src::SELECTED ? &src.sel : nullptr;
    // mode 1 (flat): one list of n*W entries (entry i*W + j = digit j of scalar i), one bucket set
    // mode 2 (endomorphism split): 2n columns of W digits
    const bool flat = mode == 1;
    const size_t ne = flat ? n * (size_t)W : (mode == 2 ? 2 * n : n);
    const int We = flat ? 1 : W;
    const sort_geom sg = sort_geometry(ne, c, We);
    const int hb = sg.hb;
    const uint32_t nbin = 1u << hb;
    // the top window sorted by the bits it really has (group_vtable.h sort_top_shift); short scalars size their windows
    // by the data and have no bound of the plan's
    const int dtop = ss ? 0 : l_sort_top_window(mode, mont, c, W, ne, nullptr);
    const uint32_t wtop = (uint32_t)We - 1u;
    // The digit pass on at most the workgroups the device holds at once, each with one LDS histogram over all its blocks
    // and one merge into the global counters (group_vtable.h sort_digit_grid).  The grid used to be 1024 workgroups or
    // more whatever the length, so a 2^20-point call paid two global atomics per scalar on the same 65 cache lines.
    const size_t lds = (size_t)We * nbin * 4;
    if (ss) {
        // packed integers: a work item is one 16-byte vector of elements, so a block may be smaller than SORT_TPB items
        // (a million bytes are 65536 items)
        const int k = ss->kind;
        const size_t items = k == 1 ? packed_items<1>(scalars, n) : k == 2 ? packed_items<2>(scalars, n) : k == 4 ? packed_items<4>(scalars, n)
                             : k == 8 ? packed_items<8>(scalars, n) : n;
#define AMDMSM_LAUNCH_SHORT(K)                                                                                              \
    do {                                                                                                                    \
        const digit_grid dg = sort_digit_grid(items, K ? 256u : (uint32_t)SORT_TPB,                                         \
                                              digit_pass_workgroups((const void*)k_sort_digits_short<K>, lds));             \
        hipLaunchKernelGGL(k_sort_digits_short<K>, dim3(dg.grid), dim3(SORT_TPB), lds, st, (const void*)scalars, n, mont, c, W, hb, \
                           dg.block, b.digits, b.stride, b.coarse, ss->limit_bits, ss->flag);                                   \
    } while (0)
        if (k == 1) AMDMSM_LAUNCH_SHORT(1);
        else if (k == 2) AMDMSM_LAUNCH_SHORT(2);
        else if (k == 4) AMDMSM_LAUNCH_SHORT(4);
        else if (k == 8) AMDMSM_LAUNCH_SHORT(8);
        else AMDMSM_LAUNCH_SHORT(0);
#undef AMDMSM_LAUNCH_SHORT
    } else if (sel) {
        const digit_grid dg = sort_digit_grid(n, SORT_TPB, digit_pass_workgroups((const void*)k_sort_digits_sel, lds));
        hipLaunchKernelGGL(k_sort_digits_sel, dim3(dg.grid), dim3(SORT_TPB), lds, st, scalars, n, mont, c, W, hb, b.digits, b.stride,
                           b.coarse, mode, sel->index, sel->offset, sel->shared_n, sel->flag, dtop);
    } else {
        const digit_grid dg = sort_digit_grid(n, SORT_TPB, digit_pass_workgroups((const void*)k_sort_digits, lds));
        hipLaunchKernelGGL(k_sort_digits, dim3(dg.grid), dim3(SORT_TPB), lds, st, scalars, n, mont, c, W, hb, b.digits, b.stride,
                           b.coarse, mode, dtop);
    }
    sort_key_t* tmp_key16 = reinterpret_cast<sort_key_t*>(b.tmp_key);   // W * stride fine keys
    const dim3 coarse_grid((unsigned)((ne + SORT_TILE - 1) / SORT_TILE), We);
    if (c <= 17)   // the bucket index has c - 1 bits
        hipLaunchKernelGGL(k_sort_coarse<unsigned short>, coarse_grid, dim3(SORT_TPB), 0, st, b.digits, ne, b.stride, c, hb, b.coarse,
                           b.cursor, b.tmp_payload, tmp_key16, dtop);
    else
        hipLaunchKernelGGL(k_sort_coarse<uint32_t>, coarse_grid, dim3(SORT_TPB), 0, st, b.digits, ne, b.stride, c, hb, b.coarse,
                           b.cursor, b.tmp_payload, tmp_key16, dtop);
    // per-chunk histograms of a bin of up to 16 chunks, where they fit beside the staging area (<= 32 KiB)
    static const bool split_hist = !(getenv("AMDMSM_SORT_SPLIT_HIST") && atoi(getenv("AMDMSM_SORT_SPLIT_HIST")) == 0);
    uint32_t perchunk_words = 0;
    if (split_hist && sg.chunk_cap >= 16384 && ((size_t)16 << sg.fb) * 4 <= 32768) perchunk_words = 16u << sg.fb;
    const size_t fine_lds = ((size_t)4 << sg.fb) * 4 + (size_t)sg.chunk_cap * 6 + (size_t)perchunk_words * 4;
    const size_t big_lds = ((size_t)4 << sg.fb) * 4 + (size_t)SORT_TILE * 4;
    // AMDMSM_SORT_REPORT=1: workgroups per CU the runtime grants the 1024-thread passes, asked once, at the first call's sizes
    static const bool reported = [&] {
        if (!(getenv("AMDMSM_SORT_REPORT") && atoi(getenv("AMDMSM_SORT_REPORT")))) return false;
        int k16 = 0, k32 = 0, kf = 0, kb = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&k16, k_sort_coarse<unsigned short>, SORT_TPB, 0);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&k32, k_sort_coarse<uint32_t>, SORT_TPB, 0);
        if (sg.chunk_cap <= 8192)
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&kf, k_sort_fine<SORT_TPB, 8>, SORT_TPB, fine_lds);
        else if (sg.chunk_cap <= 12288)
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&kf, k_sort_fine<SORT_TPB, 12>, SORT_TPB, fine_lds);
        else
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&kf, k_sort_fine<SORT_TPB, 16>, SORT_TPB, fine_lds);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&kb, k_sort_big_scatter, SORT_TPB, big_lds);
        fprintf(stderr, "[amdmsm sort] workgroups per CU: k_sort_coarse 16-bit keys %d, 32-bit keys %d; k_sort_fine<1024> "
                        "(chunk_cap %u, %zu B of LDS) %d; k_sort_big_scatter (%zu B) %d\n",
                k16, k32, sg.chunk_cap, fine_lds, kf, big_lds, kb);
        return true;
    }();
    (void)reported;
#define AMDMSM_LAUNCH_FINE(NT, PER)                                                                                          \
    hipLaunchKernelGGL((k_sort_fine<NT, PER>), dim3(nbin, We), dim3(NT), fine_lds, st, b.tmp_payload, tmp_key16, b.coarse, b.stride, c, \
                       hb, sg.chunk_cap, sg.big_thresh, sg.big_cap, perchunk_words, b.big, b.ends, b.lists, dtop)
    if (sg.chunk_cap <= 4096)
        AMDMSM_LAUNCH_FINE(256, 16);
    else if (sg.chunk_cap <= 8192)
        AMDMSM_LAUNCH_FINE(SORT_TPB, 8);
    else if (sg.chunk_cap <= 12288)
        AMDMSM_LAUNCH_FINE(SORT_TPB, 12);
    else
        AMDMSM_LAUNCH_FINE(SORT_TPB, 16);
#undef AMDMSM_LAUNCH_FINE
    hipLaunchKernelGGL(k_sort_big_hist, dim3(512), dim3(SORT_TPB), 0, st, tmp_key16, b.coarse, b.stride, c, hb, b.big, b.ends, wtop, dtop);
    hipLaunchKernelGGL(k_sort_big_scan, dim3(256), dim3(SORT_TPB), 0, st, b.coarse, c, hb, sg.big_cap, b.big, b.ends, wtop, dtop);
    hipLaunchKernelGGL(k_sort_big_scatter, dim3(512), dim3(SORT_TPB), big_lds, st, b.tmp_payload, tmp_key16, b.coarse, b.stride, c,
                       hb, sg.big_cap, b.big, b.lists, wtop, dtop);
}
void l_scalar_bits(hipStream_t st, const void* scalars, int kind, size_t n, int mont, uint32_t* out) {
    if (!n) return;
    const size_t items = kind == 1 ? packed_items<1>(scalars, n) : kind == 2 ? packed_items<2>(scalars, n)
                         : kind == 4 ? packed_items<4>(scalars, n) : kind == 8 ? packed_items<8>(scalars, n) : n;
    const dim3 grid((unsigned)std::min<size_t>((items + TPB - 1) / TPB, 4096));
    if (kind == 1) hipLaunchKernelGGL(k_scalar_bits<1>, grid, dim3(TPB), 0, st, scalars, n, mont, out);
    else if (kind == 2) hipLaunchKernelGGL(k_scalar_bits<2>, grid, dim3(TPB), 0, st, scalars, n, mont, out);
    else if (kind == 4) hipLaunchKernelGGL(k_scalar_bits<4>, grid, dim3(TPB), 0, st, scalars, n, mont, out);
    else if (kind == 8) hipLaunchKernelGGL(k_scalar_bits<8>, grid, dim3(TPB), 0, st, scalars, n, mont, out);
    else hipLaunchKernelGGL(k_scalar_bits<0>, grid, dim3(TPB), 0, st, scalars, n, mont, out);
}
void l_gather_scalars(hipStream_t st, const uint32_t* shared, size_t shared_n, const uint32_t* index, size_t offset,
                      uint32_t* flag, size_t n, uint32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_gather_scalars, dim3(blocks_for(n)), dim3(TPB), 0, st, shared, n, index, offset, shared_n, flag, out);
}
size_t l_accumulate_resident_lanes(int overlap);
// dynamic LDS that keeps one workgroup per CU out in overlap mode: with k workgroups resident by registers the
// kernel's 16 KiB of staging plus this must exceed 160 KiB / k
constexpr size_t ACC_OVERLAP_LDS = AMDMSM_ACC_WAVES >= 3 ? (160 * 1024) / AMDMSM_ACC_WAVES - 16 * 1024 + 1024 : 0;
void l_accumulate(hipStream_t st, const uint32_t* ends, const uint32_t* lists, size_t list_stride, const uint32_t* bases,
                  uint32_t* buckets, uint32_t* part_first, uint32_t* part_last, uint32_t* cont_bucket, int W, uint32_t B,
                  uint32_t S, uint32_t T, const uint32_t* endo_pts, size_t n_real, int overlap) {
    overlap = overlap && AMDMSM_OVERLAP_OK && ACC_OVERLAP_LDS;
    int sync_waves = (size_t)W * T * ACC_LANES <= 2 * l_accumulate_resident_lanes(overlap) * ACC_LANES ? 1 : 0;
    if (overlap) sync_waves = 2;   // also in long launches: the tail waves of the MSM in front must win the SIMD
    const size_t dyn_lds = overlap ? ACC_OVERLAP_LDS : 0;
#ifdef AMDMSM_ACC_TRACE
    {
        const size_t waves = (size_t)blocks_for((size_t)W * T * ACC_LANES) * TPB / 64;
        static unsigned long long* d_trace = nullptr;
        static size_t cap = 0;
        if (cap < waves) {
            if (d_trace) (void)hipFree(d_trace);
            (void)hipMalloc(&d_trace, waves * 24);
            cap = waves;
        }
        (void)hipMemsetAsync(d_trace, 0, waves * 24, st);
        hipLaunchKernelGGL(k_accumulate, dim3(blocks_for((size_t)W * T * ACC_LANES)), dim3(TPB), dyn_lds, st, ends, lists,
                           list_stride, bases, buckets, part_first, part_last, cont_bucket, W, B, S, T, endo_pts,
                           endo_pts ? (uint32_t)n_real : 0x80000000u, sync_waves, d_trace);
        if (const char* path = getenv("AMDMSM_ACC_TRACE_FILE")) {
            (void)hipStreamSynchronize(st);
            std::vector<unsigned long long> h(waves * 3);
            (void)hipMemcpy(h.data(), d_trace, waves * 24, hipMemcpyDeviceToHost);
            if (FILE* f = fopen(path, "wb")) {
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
    }
#else
    hipLaunchKernelGGL(k_accumulate, dim3(blocks_for((size_t)W * T * ACC_LANES)), dim3(TPB), dyn_lds, st, ends, lists,
                       list_stride, bases, buckets, part_first, part_last, cont_bucket, W, B, S, T, endo_pts,
                       endo_pts ? (uint32_t)n_real : 0x80000000u, sync_waves);
#endif
    // (no export pass: the readers of the records convert the limb form in registers, load_xyzz_rec)
}
void l_endo_points(hipStream_t st, const uint32_t* bases, size_t n, uint32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_endo_points, dim3(blocks_for(n * 2 * GP::DEG)), dim3(TPB), 0, st, bases, n, out);
}
void l_glv_digits(hipStream_t st, const uint32_t* scalars, size_t n, int mont, int c, int W, int32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_glv_digits, dim3(blocks_for(n)), dim3(TPB), 0, st, scalars, n, mont, c, W, out);
}
size_t l_accumulate_resident_lanes(int overlap) {
    auto query = [](size_t dyn_lds) {
        int dev = 0, cus = 256, blocks = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_accumulate, TPB, dyn_lds) != hipSuccess || blocks <= 0) blocks = 4;
        return (size_t)cus * (size_t)blocks * TPB / ACC_LANES;
    };
    static const size_t lanes = query(0);
    static const size_t lanes_overlap = (AMDMSM_OVERLAP_OK && ACC_OVERLAP_LDS) ? query(ACC_OVERLAP_LDS) : lanes;
    return overlap ? lanes_overlap : lanes;
}
void l_accumulate_fixup(hipStream_t st, const uint32_t* ends, uint32_t* buckets, uint32_t* part_first,
                        const uint32_t* part_last, const uint32_t* cont_bucket, uint32_t* queue, int W, uint32_t B,
                        uint32_t S, uint32_t T) {
    // two launches: the spans (and, in the same grid, the folding of aligned blocks inside very long spans), then both
    // queues side by side
    const unsigned fix_blocks = blocks_for((size_t)W * T * RED_LANES, 64);
    const unsigned compact_blocks = T / FIX_BLOCK >= 2 ? (unsigned)(W * (T / FIX_BLOCK - 1)) : 0u;
    hipLaunchKernelGGL(k_accumulate_fixup, dim3(fix_blocks + compact_blocks), dim3(64), 0, st, ends, part_first,
                       part_last, cont_bucket, buckets, queue, W, B, S, T, fix_blocks);
    const size_t lanes = (size_t)W * T;
    const size_t cap_mid = fixup_queue_cap_mid(lanes) / (RED_FOLD / MID_G) + 1, cap_long = fixup_queue_cap_long(lanes);
    const unsigned mid_blocks = (unsigned)(cap_mid < 8192 ? cap_mid : 8192), long_blocks = (unsigned)(cap_long < 2048 ? cap_long : 2048);
    hipLaunchKernelGGL(k_accumulate_fixup_queue, dim3(mid_blocks + long_blocks), dim3(64), 0, st, ends,
                       part_first, part_last, cont_bucket, buckets, queue, mid_blocks, lanes, B, S, T);
}
void l_reduce_segments(hipStream_t st, const uint32_t* buckets, int W, uint32_t B, uint32_t L, uint32_t* out) {
    hipLaunchKernelGGL(k_reduce_segments, dim3(blocks_for((size_t)W * (B / L) * RED_LANES, 64)), dim3(64), 0, st, buckets, W, B,
                       L, out);
}
void l_sum_butterfly(hipStream_t st, const uint32_t* in, int W, uint32_t M, uint32_t* out) {
    hipLaunchKernelGGL(k_sum_butterfly, dim3(blocks_for((size_t)W * M * RED_LANES, 64)), dim3(64), 0, st, in, W, M, out);
}
void l_sum_block(hipStream_t st, const uint32_t* in, int W, uint32_t M, uint32_t* out) {
    if (M >= 8 && M * RED_LANES <= (uint32_t)SUMW_THREADS && (M & (M - 1)) == 0) {
        hipLaunchKernelGGL(k_sum_block_wide, dim3(W), dim3(SUMW_THREADS), 0, st, in, W, M, out);
        return;
    }
    const unsigned threads = (unsigned)((M * RED_LANES + 63) / 64 * 64);
    hipLaunchKernelGGL(k_sum_block, dim3(W), dim3(threads), 0, st, in, W, M, out);
}
// rc: W * (R + 1 + C) points, planes: W * c points, out: W points (see k_bucket_sums)
void l_reduce_rowcol(hipStream_t st, const uint32_t* buckets, int W, uint32_t B, int c, uint32_t q_row, uint32_t q_col,
                     uint32_t* rc, uint32_t* planes, uint32_t* out) {
    const int h = c / 2;   // ceil((c - 1) / 2) column bits
    const uint32_t C = 1u << h, R = B >> h;
    // lanes of one sum: len / q <= RED_FOLD, q a power of two >= 1
    auto fit = [](uint32_t len, uint32_t q) {
        if (q < 1) q = 1;
        while (q & (q - 1)) q &= q - 1;
        if (q > len) q = len;
        while (len / q > RED_FOLD) q <<= 1;
        return q;
    };
    q_row = fit(C, q_row);
    q_col = fit(R, q_col);
    const size_t row_lanes = (size_t)W * (R + 1) * (C / q_row) * RED_LANES, col_lanes = (size_t)W * C * (R / q_col) * RED_LANES;
    const unsigned row_blocks = blocks_for(row_lanes, 64), col_blocks = blocks_for(col_lanes, 64);
    hipLaunchKernelGGL(k_bucket_sums, dim3(row_blocks + col_blocks), dim3(64), 0, st, buckets, W, B, h, q_row, q_col, row_blocks, rc);
    const uint32_t maxm = (C > R ? C : R) / 2;
    static const bool wide_planes = !(getenv("AMDMSM_PLANES_WIDE") && atoi(getenv("AMDMSM_PLANES_WIDE")) == 0);
    if (maxm >= 8 && wide_planes) {
        hipLaunchKernelGGL(k_plane_sums_wide, dim3((unsigned)(W * c)), dim3(SUMW_THREADS), 0, st, rc, W, c, h, planes);
    } else {
        unsigned threads = (unsigned)((maxm * RED_LANES + 63) / 64 * 64);
        threads = threads < 64 ? 64 : (threads > 256 ? 256 : threads);
        hipLaunchKernelGGL(k_plane_sums, dim3((unsigned)(W * c)), dim3(threads), 0, st, rc, W, c, h, planes);
    }
    launch_window_horner(st, planes, W, c, out);
}
void l_horner(hipStream_t st, const uint32_t* window_sums, int W, int c, int form, const uint32_t* init, uint32_t* out) {
    launch_horner(st, window_sums, W, c, form, init, out);
}
void l_horner_batch(hipStream_t st, const uint32_t* window_sums, int k, int W, int c, int form, uint32_t* const* outs) {
    horner_outs o = {};
    for (int j = 0; j < k && j < 8; ++j) o.p[j] = outs[j];
    launch_horner_batch(st, window_sums, k, W, c, form, o);
}
void l_sum_points(hipStream_t st, const uint32_t* pts, int k, int form, uint32_t* out) {
    hipLaunchKernelGGL(k_sum_points, dim3(1), dim3(64), 0, st, pts, k, form, out);
}
void l_gen_bases_seq(hipStream_t st, unsigned long long first, size_t n, uint32_t* dst) {
    if (!n) return;
    hipLaunchKernelGGL(k_gen_bases_seq, dim3(blocks_for(n)), dim3(TPB), 0, st, first, n, dst);
}
void l_export_affine(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst) {
    if (!n) return;
    hipLaunchKernelGGL(k_export_affine, dim3(blocks_for(n)), dim3(TPB), 0, st, src, n, dst);
}
void l_ffi_decode_points(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst, uint32_t* status) {
    if (!n) return;
    hipLaunchKernelGGL(k_ffi_decode_points, dim3(blocks_for(n)), dim3(TPB), 0, st, src, n, dst, status);
}
void l_ffi_decode_scalars(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst, uint32_t* status) {
    if (!n) return;
    hipLaunchKernelGGL(k_ffi_decode_scalars, dim3(blocks_for(n)), dim3(TPB), 0, st, src, n, dst, status);
}
void l_ffi_encode_point(hipStream_t st, const uint32_t* src_xyz, uint32_t* dst) {
    hipLaunchKernelGGL(k_ffi_encode_point, dim3(1), dim3(64), 0, st, src_xyz, dst);
}
void l_disk_decode(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst) {
    if (!n) return;
    hipLaunchKernelGGL(k_disk_decode, dim3(blocks_for(n)), dim3(TPB), 0, st, src, n, dst);
}
void l_disk_decode_compressed(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst, uint32_t* status) {
    if (!n) return;
    hipLaunchKernelGGL(k_disk_decode_compressed, dim3(blocks_for(n, 64)), dim3(64), 0, st, src, n, dst, status);
}
// the encoders stride: at most DISK_ENCODE_BLOCKS workgroups, each lane taking records TPB * grid apart
constexpr size_t DISK_ENCODE_BLOCKS = 8192;
void l_disk_encode(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst) {
    if (!n) return;
    const unsigned blocks = (unsigned)std::min<size_t>((n + TPB - 1) / TPB, DISK_ENCODE_BLOCKS);
    hipLaunchKernelGGL(k_disk_encode, dim3(blocks), dim3(TPB), 0, st, src, n, dst);
}
void l_disk_encode_compressed(hipStream_t st, const uint32_t* src, size_t n, uint32_t* dst) {
    if (!n) return;
    const unsigned blocks = (unsigned)std::min<size_t>((n + TPB - 1) / TPB, DISK_ENCODE_BLOCKS);
    hipLaunchKernelGGL(k_disk_encode_compressed, dim3(blocks), dim3(TPB), 0, st, src, n, dst);
}
// table: outerc * 2^window Jacobian points of scratch, gouter: outerc points, table_aff: outerc * 2^window
// compact affine records (what k_fb_exp reads).  build_table = 0: table_aff already holds the table of this
// (g, scalar_size, window) -- the caller keeps it between calls.
#if AMDMSM_ACC_RR
template <class G>
bool launch_fb_exp_rr(hipStream_t st, const uint32_t* table_aff, const uint32_t* scalars, size_t n, int mont, const uint32_t* coeff,
                      int scalar_size, int window, int form, uint32_t* out) {
    if constexpr (G::DEG == 1) {
        if (window < 32) {
            hipLaunchKernelGGL(k_fb_exp_rr<G>, dim3(blocks_for(n)), dim3(TPB), 0, st, table_aff, scalars, n, mont, coeff, scalar_size,
                               window, form, out);
            return true;
        }
    }
    return false;
}
#endif
void l_fixed_base_exp(hipStream_t st, const uint32_t* g_xyz, int scalar_size, int window, const uint32_t* scalars, size_t n,
                      int mont, const uint32_t* coeff, int form, uint32_t* gouter, uint32_t* table, uint32_t* table_aff,
                      int build_table, uint32_t* out) {
    const int outerc = (scalar_size + window - 1) / window;
    if (build_table) {
        hipLaunchKernelGGL(k_fb_gouter, dim3(1), dim3(64), 0, st, g_xyz, outerc, window, gouter);
        for (int level = 0; level < window; ++level) {
            const size_t per_level = level == 0 ? 2 : ((size_t)1 << level);
            hipLaunchKernelGGL(k_fb_table_level, dim3(blocks_for((size_t)outerc * per_level)), dim3(TPB), 0, st, gouter, outerc,
                               window, scalar_size, level, table);
        }
        // (entries past the shorter last row are never addressed by k_fb_exp; they read as whatever the scratch held,
        // so the row is cleared first: an all-zero Jacobian record has Z == 0 = infinity)
        const size_t entries = (size_t)outerc << window;
        hipLaunchKernelGGL(k_fb_table_affine, dim3(blocks_for((entries + FB_NORM_K - 1) / FB_NORM_K)), dim3(TPB), 0, st, table,
                           entries, table_aff);
    }
    if (n) {
#if AMDMSM_ACC_RR
        if (launch_fb_exp_rr<GP>(st, table_aff, scalars, n, mont, coeff, scalar_size, window, form, out)) return;
#endif
        hipLaunchKernelGGL(k_fb_exp, dim3(blocks_for(n)), dim3(TPB), 0, st, table_aff, scalars, n, mont, coeff, scalar_size,
                           window, form, out);
    }
}
void l_field_op(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_field_op, dim3(blocks_for(n)), dim3(TPB), 0, st, op, a, b, out, n);
}
void l_field_probe(hipStream_t st, int impl, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                   uint32_t* out, uint32_t* flag, size_t n) {
    if (!n) return;
    if (impl) hipLaunchKernelGGL(k_field_probe<EI>, dim3(blocks_for(n)), dim3(TPB), 0, st, op, a, b, c, d, out, flag, n);
    else hipLaunchKernelGGL(k_field_probe<E>, dim3(blocks_for(n)), dim3(TPB), 0, st, op, a, b, c, d, out, flag, n);
}
void l_xyzz_probe(hipStream_t st, int impl, int op, const uint32_t* acc, const uint32_t* pt, uint32_t* out, size_t n) {
    if (!n) return;
    if (impl) hipLaunchKernelGGL(k_xyzz_probe<EI>, dim3(blocks_for(n)), dim3(TPB), 0, st, op, acc, pt, out, n);
    else hipLaunchKernelGGL(k_xyzz_probe<E>, dim3(blocks_for(n)), dim3(TPB), 0, st, op, acc, pt, out, n);
}
#if AMDMSM_ACC_RR
void l_rr_probe(hipStream_t st, int op, int k, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                const uint32_t* w, int32_t* out, uint32_t* outw, uint32_t* flag, size_t n) {
    if (!n) return;
    const dim3 grid(blocks_for(n * RRP_LANES));
    if (op < RRPROBE_NORM) hipLaunchKernelGGL(k_rr_probe<0>, grid, dim3(TPB), 0, st, op, k, a, b, c, d, w, out, outw, flag, n);
    else hipLaunchKernelGGL(k_rr_probe<1>, grid, dim3(TPB), 0, st, op, k, a, b, c, d, w, out, outw, flag, n);
}
void l_xyzz_rr_probe(hipStream_t st, int op, const int32_t* acc, const int32_t* sec, const uint32_t* pt, const uint32_t* fin,
                     int32_t* out, uint32_t* outw, uint32_t* fout, size_t n) {
    if (!n) return;
    const dim3 grid(blocks_for(n * RRP_LANES));
    if (op < XRRPROBE_DBL_RHO)
        hipLaunchKernelGGL(k_xyzz_rr_probe<0>, grid, dim3(TPB), 0, st, op, acc, sec, pt, fin, out, outw, fout, n);
    else if (op < XRRPROBE_JAC_DBL)
        hipLaunchKernelGGL(k_xyzz_rr_probe<1>, grid, dim3(TPB), 0, st, op, acc, sec, pt, fin, out, outw, fout, n);
    else
        hipLaunchKernelGGL(k_xyzz_rr_probe<2>, grid, dim3(TPB), 0, st, op, acc, sec, pt, fin, out, outw, fout, n);
}
#endif
void l_group_op(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, int form) {
    if (!n) return;
    hipLaunchKernelGGL(k_group_op, dim3(blocks_for(n)), dim3(TPB), 0, st, op, a, b, out, n, form);
}
void l_digits(hipStream_t st, const uint32_t* scalars, size_t n, int mont, int c, int W, int32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_digits, dim3(blocks_for(n)), dim3(TPB), 0, st, scalars, n, mont, c, W, out);
}
void l_mul_bench(hipStream_t st, uint32_t* inout, size_t nthreads, int iters, int inline_variant) {
    if (!nthreads) return;
#if AMDMSM_BENCH_BOTH
    if (inline_variant) {
        hipLaunchKernelGGL(k_mul_bench<true>, dim3(blocks_for(nthreads)), dim3(TPB), 0, st, inout, nthreads, iters);
        return;
    }
#endif
    hipLaunchKernelGGL(k_mul_bench<false>, dim3(blocks_for(nthreads)), dim3(TPB), 0, st, inout, nthreads, iters);
}
void l_madd_bench(hipStream_t st, const uint32_t* pts, uint32_t* out, size_t nthreads, int iters, int inline_variant) {
    if (!nthreads) return;
    if (inline_variant == 2) {
        hipLaunchKernelGGL(k_xyzz_madd_bench<EH>, dim3(blocks_for(nthreads)), dim3(TPB), 0, st, pts, out, nthreads, iters);
        return;
    }
#if AMDMSM_BENCH_BOTH
    if (inline_variant) {
        hipLaunchKernelGGL(k_madd_bench<EI>, dim3(blocks_for(nthreads)), dim3(TPB), 0, st, pts, out, nthreads, iters);
        return;
    }
#endif
    hipLaunchKernelGGL(k_madd_bench<E>, dim3(blocks_for(nthreads)), dim3(TPB), 0, st, pts, out, nthreads, iters);
}
void l_smv_table(hipStream_t st, const uint32_t* bases, size_t n, uint32_t* tmp, uint32_t* table) {
    if (!n) return;
    hipLaunchKernelGGL(k_smv_table, dim3(blocks_for(n)), dim3(TPB), 0, st, bases, n, tmp, table);
}
void l_smv_ladder(hipStream_t st, const uint32_t* table, size_t n, const uint32_t* scalars, int mont, int form, uint32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_smv_ladder, dim3(blocks_for(n)), dim3(TPB), 0, st, table, n, scalars, mont, form, out);
}
void l_seg_digits(hipStream_t st, const uint32_t* scalars, size_t n, int mont, uint32_t* digits) {
    if (!n) return;
    hipLaunchKernelGGL(k_seg_digits, dim3(blocks_for(n)), dim3(TPB), 0, st, scalars, n, mont, digits);
}
void l_seg_accumulate(hipStream_t st, const uint32_t* table, size_t nt, const uint32_t* digits, const uint32_t* slices,
                      size_t n_slices, uint32_t* sums) {
    if (!n_slices) return;
    const size_t lanes = n_slices * SMV_DIGITS;
    hipLaunchKernelGGL(k_seg_accumulate, dim3(blocks_for(lanes)), dim3(TPB), 0, st, table, nt, (const signed char*)digits,
                       (const uint4*)slices, lanes, sums);
}
void l_seg_fold(hipStream_t st, const uint32_t* sums, const uint32_t* seg_first, size_t m, uint32_t* winsum) {
    if (!m) return;
    const size_t lanes = m * SMV_DIGITS;
    hipLaunchKernelGGL(k_seg_fold, dim3(blocks_for(lanes)), dim3(TPB), 0, st, sums, seg_first, lanes, winsum);
}
void l_seg_horner(hipStream_t st, const uint32_t* winsum, size_t m, int form, uint32_t* out) {
    if (!m) return;
    launch_seg_horner(st, winsum, m, form, out);
}
void l_fold_digits(hipStream_t st, const uint32_t* scalars_host, int k, int mont, int glv, int W, uint32_t* digits) {
    if (k < 1 || k > FOLD_MAX_K) return;
    fold_scalars sc = {};
    std::copy(scalars_host, scalars_host + (size_t)k * FRW, sc.w);
    hipLaunchKernelGGL(k_fold_digits, dim3(1), dim3(64), 0, st, sc, k, mont, GP::HAS_ENDO ? glv : 0, W, digits);
}
void l_fold_ladder(hipStream_t st, const uint32_t* tables, size_t n, const uint32_t* digits, int rows, int glv, int W, int form,
                   uint32_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(k_fold_ladder, dim3(blocks_for(n)), dim3(TPB), 0, st, tables, n, digits, rows, GP::HAS_ENDO ? glv : 0, W,
                       form, out);
}
void l_fft_gather(hipStream_t st, const uint32_t* in, size_t b0, size_t cn, int rsh, uint32_t* dst) {
    if (!cn) return;
    hipLaunchKernelGGL(k_fft_gather, dim3(blocks_for(cn * (AFFW / 4))), dim3(TPB), 0, st, in, b0, cn, rsh, dst);
}
void l_fft_butterfly(hipStream_t st, const uint32_t* table, size_t cn, const uint32_t* in, size_t b0, int rsh,
                     const uint32_t* twiddles, int mont, size_t half, uint32_t* out) {
    if (!cn) return;
    if (table)
        hipLaunchKernelGGL(k_fft_butterfly<true>, dim3(blocks_for(cn)), dim3(TPB), 0, st, table, cn, in, b0, rsh, twiddles, mont,
                           half, out);
    else
        hipLaunchKernelGGL(k_fft_butterfly<false>, dim3(blocks_for(cn)), dim3(TPB), 0, st, table, cn, in, b0, rsh, twiddles, mont,
                           half, out);
}

#include "group_matrix.inc"

const group_vtable g_vt = {
    // constants of the group
    .curve = GP::CURVE, .group = GP::GROUP, .fr_words = FRW, .el_words = EW, .fq_words = FQ::N, .fr_bits = FR::BITS,
    .projective = GP::LIBFF_PROJECTIVE ? 1 : 0, .reduce_fold = (int)RED_FOLD, .bucket_words = ZZS,
    .fr_one_mont = FR::R, .fr_modulus = FR::P,
    .has_endomorphism = GP::HAS_ENDO ? 1 : 0, .coeff_a_nonzero = GP::COEFF_A != 0 ? 1 : 0,
    .glv_bound_log2_x1000 = GLV::BOUND_LOG2_X1000, .prime_order = GP::SUBGROUP_CHECK == 0 ? 1 : 0, .glv_lambda = GLV::LAMBDA,
    // import / export / codecs
    .import_bases = l_import_bases, .export_affine = l_export_affine, .gen_bases_seq = l_gen_bases_seq,
    .endo_points = l_endo_points, .precompute_table = l_precompute_table,
    .ffi_decode_points = l_ffi_decode_points, .ffi_decode_scalars = l_ffi_decode_scalars, .ffi_encode_point = l_ffi_encode_point,
    .disk_decode = l_disk_decode, .disk_decode_compressed = l_disk_decode_compressed,
    .disk_encode = l_disk_encode, .disk_encode_compressed = l_disk_encode_compressed,
    // digits and sort
    .scalar_stats = l_scalar_stats, .scalar_bits = l_scalar_bits, .gather_scalars = l_gather_scalars,
    .count = l_count, .scatter = l_scatter, .sort = l_sort, .sort_top_window = l_sort_top_window,
    // accumulate and fix-up
    .accumulate = l_accumulate, .accumulate_resident_lanes = l_accumulate_resident_lanes,
    .accumulate_overlap_ok = (AMDMSM_OVERLAP_OK && ACC_OVERLAP_LDS) ? 1 : 0, .accumulate_fixup = l_accumulate_fixup,
    // reduction and Horner
    .reduce_segments = l_reduce_segments, .sum_butterfly = l_sum_butterfly, .sum_block = l_sum_block,
    .reduce_rowcol = l_reduce_rowcol, .horner = l_horner, .horner_batch = l_horner_batch, .sum_points = l_sum_points,
    // fixed-base
    .fixed_base_exp = l_fixed_base_exp,
    // point-vector entries
    .smv_entries = SMV_T, .smv_table = l_smv_table, .smv_ladder = l_smv_ladder,
    .seg_windows = SMV_DIGITS, .seg_digit_stride = SMV_DS, .seg_digits = l_seg_digits, .seg_accumulate = l_seg_accumulate,
    .seg_fold = l_seg_fold, .seg_horner = l_seg_horner,
    .fold_digit_stride = SMV_DS, .fold_digits = l_fold_digits, .fold_ladder = l_fold_ladder,
    .fft_gather = l_fft_gather, .fft_butterfly = l_fft_butterfly,
    .gm_gather = l_gm_gather, .gm_apply = l_gm_apply, .gm_combine = l_gm_combine,
    // test hooks and probes
    .field_op = l_field_op, .group_op = l_group_op, .digits = l_digits, .glv_digits = l_glv_digits,
    .mul_bench = l_mul_bench, .madd_bench = l_madd_bench, .field_probe = l_field_probe, .xyzz_probe = l_xyzz_probe,
#if AMDMSM_ACC_RR
    .rr_probe = l_rr_probe, .xyzz_rr_probe = l_xyzz_rr_probe, .rr_probe_first_reduced = RRP_FIRST_REDUCED ? 1 : 0,
#endif
};

}  // namespace

const group_vtable* AMDMSM_VT() { return &g_vt; }

}  // namespace amdmsm
