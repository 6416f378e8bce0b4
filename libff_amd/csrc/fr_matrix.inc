// Sparse matrix times Fr vector (amdmsm_fr_matrix_apply): the kernels over the resident form of fr_matrix_layout.h and the
// straightforward CSR kernel behind AMDMSM_FR_MATRIX_NAIVE=1.  Included by fr_ntt.hip inside its anonymous namespace,
// once per scalar field; DESIGN section 19.
//
// Record forms.  The side array holds the general coefficients as Montgomery residues c R.  A Montgomery product with
// a record of x then gives c x in whatever form x is in (c R * x / R), and entries of coefficient 1 and r - 1 add and
// subtract records as they stand, so one kernel serves plain and Montgomery vectors and never converts.

// ---- the bounds ------------------------------------------------------------------------------------------------------
// A row's general products are summed unreduced, FRM_T of them to a chain, in `acc`, 2N words: with c, x <= r - 1 the sum
// is at most T (r - 1)^2, and one Montgomery reduction of it gives (sum + m r) / R < T r^2 / R + r with m < R.  T is the
// largest count (1024 at the most) for which that stays below R = 2^(32N), by the modulus's top word as fp_dot_lz takes
// its bound:  r / R < (top + 1) / 2^32 =: u,  so  T r^2 / R + r < (T u + 1) r < R  where  T u + 1 < 1 / u.  Then the sum
// itself is below R^2 - r R: it fits the 2N words, and the carry out of the last column is zero.  The reduced chain --
// any value below R, not below r -- is added into `sum`, N words and a carry word, as are the records of the +-1
// entries (r - x for a subtraction: below R for x <= r); a wave job has at most 2^20 entries (the largest t_split) and
// adds as many chains at the most, and the 64 lanes' sums are then added up: the carry word holds the count many times
// over.  At the row's end sum = lo + hi 2^(32N) becomes canonical as lo * (R mod r) / R + hi * (R^2 mod r) / R, two
// Montgomery products of an operand below R by one below r: each below 2r before its one conditional subtraction.
constexpr uint32_t frm_chunk_len() {
    const double u = ((double)FR::P[N - 1] + 1.0) / 4294967296.0;
    double t = (1.0 / u - 1.0) / u;
    if (t > 1024.0) t = 1024.0;
    uint32_t T = (uint32_t)t;
    while (T > 1 && !((double)T * u + 1.0 < 1.0 / u)) --T;
    return T;
}
constexpr uint32_t FRM_T = frm_chunk_len();
static_assert(FRM_T >= 1 && (double)FRM_T * (((double)FR::P[N - 1] + 1.0) / 4294967296.0) + 1.0 <
                                4294967296.0 / ((double)FR::P[N - 1] + 1.0),
              "a reduced chain of FRM_T products must fit N words");

// acc += a * b, column by column (product scanning, the carry in (lo, hi))
template <int K>
AMDMSM_DEV void frm_mac_column(uint64_t& lo, uint32_t& hi, uint32_t (&acc)[2 * N], const uint32_t* a, const uint32_t* b) {
    const uint64_t s = lo + acc[K];
    hi += s < lo ? 1u : 0u;
    lo = s;
    if constexpr (K < N) mac_range_vv<K, 0, K + 1>(lo, hi, a, b);
    else mac_range_vv<K, K - N + 1, N>(lo, hi, a, b);
    acc[K] = (uint32_t)lo;
    lo = (lo >> 32) | ((uint64_t)hi << 32);
    hi = 0;
    if constexpr (K + 1 < 2 * N) frm_mac_column<K + 1>(lo, hi, acc, a, b);
}
AMDMSM_DEV void frm_mac(uint32_t (&acc)[2 * N], const F& a, const F& b) {
    uint64_t lo = 0;
    uint32_t hi = 0;
    frm_mac_column<0>(lo, hi, acc, a.v, b.v);   // no carry leaves column 2N - 1 (the bound above)
}

// t = acc / R mod r as a value below R: the reduction half of fp_mul_column on a given 2N-word integer
template <int K>
AMDMSM_DEV void frm_redc_column(uint64_t& lo, uint32_t& hi, uint32_t* m, uint32_t* t, const uint32_t (&acc)[2 * N]) {
    const uint64_t s = lo + acc[K];
    hi += s < lo ? 1u : 0u;
    lo = s;
    if constexpr (K < N) {
        mac_range_vs<FR, K, 0, K>(lo, hi, m);
        m[K] = (uint32_t)lo * FR::INV;
        mac_chain<1>::vs(lo, hi, m[K], FR::P[0]);
    } else {
        mac_range_vs<FR, K, K - N + 1, N>(lo, hi, m);
        t[K - N] = (uint32_t)lo;
    }
    lo = (lo >> 32) | ((uint64_t)hi << 32);
    hi = 0;
    if constexpr (K + 1 < 2 * N) frm_redc_column<K + 1>(lo, hi, m, t, acc);
}
// sum += acc / R (mod r, below R); acc = 0
AMDMSM_DEV void frm_fold_chain(uint32_t (&sum)[N + 1], uint32_t (&acc)[2 * N]) {
    uint32_t m[N], t[N];
    uint64_t lo = 0;
    uint32_t hi = 0;
    frm_redc_column<0>(lo, hi, m, t, acc);
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) sum[i] = addc32(sum[i], t[i], carry);
    sum[N] += carry;
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) acc[i] = 0;
}
AMDMSM_DEV void frm_add_rec(uint32_t (&sum)[N + 1], const F& x, bool negate) {
    uint32_t v[N];
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint32_t d = subb32(FR::P[i], x.v[i], borrow);
        v[i] = negate ? d : x.v[i];
    }
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) sum[i] = addc32(sum[i], v[i], carry);
    sum[N] += carry;
}
// the canonical record of sum
AMDMSM_DEV void frm_canon(F& r, const uint32_t (&sum)[N + 1]) {
    F lo, k;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        lo.v[i] = sum[i];
        k.v[i] = FR::R[i];
    }
    fp_mul(r, lo, k);
    if (sum[N]) {
        F hi;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            hi.v[i] = i ? 0u : sum[N];
            k.v[i] = FR::R2[i];
        }
        fp_mul(hi, hi, k);
        fp_add(r, r, hi);
    }
}

// ---- the resident form -------------------------------------------------------------------------------------------------
// One wave per job; the waves past the jobs write the zero records n_rows .. n_out - 1, one per lane.  Every index comes
// from the arrays the load built (columns < n_cols <= n_x, rows < n_rows <= n_out, partials < n_partials) and none from
// the vector: a record of x that is no field element changes values, never an address.
__global__ void __launch_bounds__(TPB) k_frm_apply(const frm_args a) {
    const uint32_t lane = threadIdx.x & (FRM_LANES - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (TPB / FRM_LANES) + threadIdx.x / FRM_LANES);
    if (wave >= a.n_desc) {
        const size_t i = a.n_rows + (size_t)(wave - a.n_desc) * FRM_LANES + lane;
        if (i < a.n_out) {
            F z;
            fp_set_zero(z);
            rec_store(a.out, i, z);
        }
        return;
    }
    const frm_desc d = a.desc[wave];
    const uint32_t mode = d.dest >> FRM_MODE_SHIFT, dest = d.dest & FRM_DEST_MASK;
    const uint32_t* words = a.words + (size_t)d.base64 * FRM_LANES + lane;
    uint32_t sum[N + 1], acc[2 * N];
#pragma unroll
    for (int i = 0; i <= N; ++i) sum[i] = 0;
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) acc[i] = 0;
    uint32_t chain = 0, rank0 = d.gen_base;
    for (uint32_t j = 0; j < d.steps; ++j) {
        const uint32_t w = words[(size_t)j * FRM_LANES];
        const uint32_t cls = w >> FRM_COL_BITS;
        const uint64_t gen = __ballot(cls == FRM_GEN);
        if (cls != FRM_PAD) {
            F x;
            rec_load(x, a.x, w & FRM_COL_MASK);
            if (cls == FRM_GEN) {
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(gen >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)gen, 0u));
                F c;
                rec_load(c, a.coef, (size_t)rank0 + below);
                frm_mac(acc, c, x);
                if (++chain == FRM_T) {
                    frm_fold_chain(sum, acc);
                    chain = 0;
                }
            } else {
                frm_add_rec(sum, x, cls == FRM_MINUS);
            }
        }
        rank0 += (uint32_t)__popcll(gen);
    }
    if (chain) frm_fold_chain(sum, acc);
    if (mode == FRM_MODE_LANES) {
        const uint32_t row = a.lane_rows[(size_t)dest * FRM_LANES + lane];
        if (row != FRM_NO_ROW) {
            F r;
            frm_canon(r, sum);
            rec_store(a.out, row, r);
        }
        return;
    }
    // the 64 sums into lane 0: N + 1 words and carries, at most 64 times a lane's sum
#pragma unroll
    for (int s = FRM_LANES / 2; s; s >>= 1) {
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) sum[i] = addc32(sum[i], __shfl_xor(sum[i], s), carry);
        sum[N] += __shfl_xor(sum[N], s) + carry;
    }
    if (lane == 0) {
        F r;
        frm_canon(r, sum);
        rec_store(mode == FRM_MODE_PART ? a.partial : a.out, dest, r);
    }
}

// out[row] = the sum of the row's partials, one lane per split row
__global__ void __launch_bounds__(TPB) k_frm_combine(const frm_comb* comb, uint32_t n_comb, const uint32_t* partial, uint32_t* out) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n_comb) return;
    const frm_comb c = comb[i];
    F r, v;
    rec_load(r, partial, c.first);
    for (uint32_t p = 1; p < c.count; ++p) {
        rec_load(v, partial, (size_t)c.first + p);
        fp_add(r, r, v);
    }
    rec_store(out, c.row, r);
}

// ---- AMDMSM_FR_MATRIX_NAIVE=1: one lane per row of the caller's CSR, a product and an addition per entry ------------------
__global__ void __launch_bounds__(TPB) k_frm_naive(size_t n_rows, size_t n_out, const uint64_t* offsets, const uint32_t* cols,
                                                   const uint32_t* coef, const uint32_t* x, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_out) return;
    F r;
    fp_set_zero(r);
    if (i < n_rows) {
        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) {
            F c, v;
            rec_load(c, coef, k);
            rec_load(v, x, cols[k]);
            fp_mul(v, v, c);
            fp_add(r, r, v);
        }
    }
    rec_store(out, i, r);
}

void l_matrix_apply(hipStream_t st, const frm_args& a) {
    const size_t tail = a.n_out - a.n_rows;
    const size_t waves = (size_t)a.n_desc + (tail + FRM_LANES - 1) / FRM_LANES, per = TPB / FRM_LANES;
    if (waves) hipLaunchKernelGGL(k_frm_apply, dim3((unsigned)((waves + per - 1) / per)), dim3(TPB), 0, st, a);
    if (a.n_comb)
        hipLaunchKernelGGL(k_frm_combine, dim3((a.n_comb + TPB - 1) / TPB), dim3(TPB), 0, st, a.comb, a.n_comb, a.partial, a.out);
}

void l_matrix_naive(hipStream_t st, size_t n_rows, size_t n_out, const uint64_t* d_offsets, const uint32_t* d_cols,
                    const uint32_t* d_coef, const uint32_t* d_x, uint32_t* d_out) {
    if (!n_out) return;
    hipLaunchKernelGGL(k_frm_naive, dim3((unsigned)((n_out + TPB - 1) / TPB)), dim3(TPB), 0, st, n_rows, n_out, d_offsets, d_cols,
                       d_coef, d_x, d_out);
}
