// Transforms over libfqfft's step radix-2 domain of m = B + S points (B = 2^log_b, S = 2^log_s, S < B) and the division
// by the vanishing polynomial on a coset (amdmsm_fr_domain_fft, amdmsm_fr_domain_divide_by_z): the sweeps in front of and
// behind the radix-2 passes of k_fr_fft_pass, which run unchanged on the B and on the S records.  Included by fr_ntt.hip
// inside its anonymous namespace, once per scalar field; DESIGN section 22.
//
// With K = B / S, w a primitive 2B-th root of unity and a'_i = g^i a_i, the forward transform is the size-B transform of
//     c_i = a'_i + a'_(B+i) (i < S),  a'_i (S <= i < B)
// and the size-S transform of the column sums e_i = sum over j < K of d_(i + j S) of
//     d_i = w^i (a'_i - a'_(B+i)) (i < S),  w^i a'_i (S <= i < B),
// that is of a K x S matrix in row-major order.  The inverse needs the same sums of w^i U0_i over the rows 1 .. K - 1.
//
// k_frd_sweep reads every record of that matrix once.  A workgroup takes a tile of W = min(S, 256) columns and
// R0 * iters rows: its 256 lanes are R0 = 256 / W rows of W neighbouring records, so every load of a wave is contiguous
// whether the columns are many and short (S >= 256: a lane walks `iters` rows of its column) or few and long (S = 1: 256
// lanes share the one column); each lane keeps one running sum, the R0 sums of a column meet in LDS, and the tile leaves
// W partial sums.  While more than one row of partial sums is left, the same kernel sums those (FRD_REDUCE), launch after
// launch in stream order: no workgroup waits for another and no record is added to in global memory.  Field addition is
// exact, so the order of the additions does not show in the canonical result.
// Every index comes from log_b, log_s, rows and the launch geometry, none from a record.

constexpr uint32_t FRD_LO = 1u << FRD_LO_LOG2;

AMDMSM_DEV void frd_red_put(uint2 (*red)[TPB], uint32_t l, const F& a) {
#pragma unroll
    for (int w = 0; w < N / 2; ++w) red[w][l] = make_uint2(a.v[2 * w], a.v[2 * w + 1]);
}
AMDMSM_DEV void frd_red_get(F& r, const uint2 (*red)[TPB], uint32_t l) {
#pragma unroll
    for (int w = 0; w < N / 2; ++w) {
        const uint2 v = red[w][l];
        r.v[2 * w] = v.x;
        r.v[2 * w + 1] = v.y;
    }
}
// v *= g^i, from the two tables g^c (c < 2^10) and g^(2^10 k)
AMDMSM_DEV void frd_coset(F& v, const uint32_t* g_lo, const uint32_t* g_hi, size_t i) {
    F f;
    rec_load(f, g_lo, i & (FRD_LO - 1));
    fp_mul(v, v, f);
    rec_load(f, g_hi, i >> FRD_LO_LOG2);
    fp_mul(v, v, f);
}

template <int MODE>
__global__ void __launch_bounds__(TPB) k_frd_sweep(const frd_sweep a) {
    __shared__ uint2 red[N / 2][TPB];
    const uint32_t tid = threadIdx.x;
    const int lw = a.log_w, ls = a.log_s;
    const uint32_t W = 1u << lw, R0 = TPB >> lw;
    // the grid is one-dimensional: S / W column tiles next to each other, then the next block of rows
    const uint32_t ctile = blockIdx.x & ((1u << (ls - lw)) - 1), rblock = blockIdx.x >> (ls - lw);
    const uint32_t col = (ctile << lw) | (tid & (W - 1)), lrow = tid >> lw;
    const uint32_t row0 = rblock * (R0 * a.iters) + lrow;
    // the lane's rows row0, row0 + R0, ...: a trip count known up front, so that the loads of neighbouring trips overlap
    uint32_t trips = row0 < a.rows ? (a.rows - row0 + R0 - 1) / R0 : 0;
    if (trips > a.iters) trips = a.iters;
    F acc;
    fp_set_zero(acc);
#pragma unroll 2
    for (uint32_t it = 0; it < trips; ++it) {
        const uint32_t j = row0 + it * R0;
        const size_t i = ((size_t)j << ls) | col;
        if constexpr (MODE == FRD_REDUCE) {
            F x;
            rec_load(x, a.in, i);
            fp_add(acc, acc, x);
        } else if constexpr (MODE == FRD_FOLD) {
            F x, d, w;
            rec_load(x, a.in, i);
            rec_load(w, a.tw, i);
            if (a.plain) fp_to_mont(x, x);
            if (a.g_lo) frd_coset(x, a.g_lo, a.g_hi, i);
            d = x;
            if (j == 0) {   // i < S: the record B + i belongs to this lane alone
                const size_t i2 = ((size_t)1 << a.log_b) + i;
                F y;
                rec_load(y, a.in, i2);
                if (a.plain) fp_to_mont(y, y);
                if (a.g_lo) frd_coset(y, a.g_lo, a.g_hi, i2);
                fp_sub(d, x, y);
                fp_add(x, x, y);
            }
            if (j == 0 || a.store) rec_store(a.out, i, x);
            fp_mul(d, d, w);
            fp_add(acc, acc, d);
        } else {   // FRD_MERGE: row 0 is k_frd_combine's
            if (j == 0) continue;
            F x, w;
            rec_load(x, a.in, i);
            rec_load(w, a.tw, i);
            fp_mul(w, w, x);
            fp_add(acc, acc, w);
            if (a.store) {
                if (a.g_lo) frd_coset(x, a.g_lo, a.g_hi, i);
                if (a.plain) fp_from_mont(x, x);
                rec_store(a.out, i, x);
            }
        }
    }
    // lane l = row * W + column: the lanes l + h, h a multiple of W, hold the same column
    frd_red_put(red, tid, acc);
    __syncthreads();
    for (uint32_t h = TPB / 2; h >= W; h >>= 1) {
        if (tid < h) {
            F o;
            frd_red_get(o, red, tid + h);
            fp_add(acc, acc, o);
            frd_red_put(red, tid, acc);
        }
        __syncthreads();
    }
    if (tid < W) rec_store(a.sums, ((size_t)rblock << ls) | col, acc);
}

// The inverse's row 0, i < S, once the sums t_i of w^(i + j S) U0_(i + j S) over j = 1 .. K - 1 are there:
//     v = w^-i (U1_i - t_i),  a_i = g^-i (U0_i + v) / 2,  a_(B+i) = g^-(B+i) (U0_i - v) / 2
// with w^-i = -w^(B - i) for i > 0 (w^B = -1), so that the B powers of w serve both directions.
__global__ void __launch_bounds__(TPB) k_frd_combine(const frd_combine a) {
    const size_t S = (size_t)1 << a.log_s, B = (size_t)1 << a.log_b;
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= S) return;
    F u0, u1, t, half;
    rec_copy(half, a.half);
    rec_load(u0, a.out, i);
    rec_load(u1, a.out, B + i);
    rec_load(t, a.sums, i);
    if (i) {
        F w;
        rec_load(w, a.tw, B - i);
        fp_sub(t, t, u1);
        fp_mul(t, t, w);
    } else {
        fp_sub(t, u1, t);
    }
    fp_mul(t, t, half);
    fp_mul(u0, u0, half);
    fp_add(u1, u0, t);
    fp_sub(u0, u0, t);
    if (a.g_lo) {
        frd_coset(u1, a.g_lo, a.g_hi, i);
        frd_coset(u0, a.g_lo, a.g_hi, B + i);
    }
    if (a.plain) {
        fp_from_mont(u1, u1);
        fp_from_mont(u0, u0);
    }
    rec_store(a.out, i, u1);
    rec_store(a.out, B + i, u0);
}

// den[k] -= c in place: the K denominators (g^B - 1) (g^S w^(2 S k) - w^S) from the powers the host asked for
__global__ void __launch_bounds__(TPB) k_frd_den(size_t n, uint32_t* den, const fr_rec_arg c) {
    const size_t k = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= n) return;
    F x, cc;
    rec_copy(cc, c.v);
    rec_load(x, den, k);
    fp_sub(x, x, cc);
    rec_store(den, k, x);
}

// out[j] = in[j] * inv[j mod K] below B, in[j] * tail from B on; the factors are Montgomery residues, which leaves a
// record in the form it came in
__global__ void __launch_bounds__(TPB) k_frd_divide(size_t m, size_t B, size_t kmask, const uint32_t* in, const uint32_t* inv,
                                                    const fr_rec_arg tail, uint32_t* out) {
    F tl;
    rec_copy(tl, tail.v);
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (size_t)gridDim.x * TPB) {
        F x, f = tl;
        rec_load(x, in, j);
        if (j < B) rec_load(f, inv, j & kmask);
        fp_mul(x, x, f);
        rec_store(out, j, x);
    }
}

// The Lagrange vector at t, DESIGN section 24.  x_j = w^e with w the root of order O = 2^log_o and e = j (basic), 2 j
// (step, j < B) or 1 + 2 K (j - B) (step, the tail: sigma = w^(2 K)); the table holds w^i for i < O / 2 and w^(O / 2) is
// -1, so w^i is tw[i] or -tw[i - O / 2].  Record j is the denominator
//     1 / L_j(t) = (t / x_j - 1) f_j,   f_j = kden[j mod K] (step, j < B) or tail,
// which the batch inversion turns into L_j(t); with Z(t) = 0 (UNIT) it is the vector itself, 1 where x_j = t.
// Every index comes from log_b, log_s, log_o and the launch geometry, none from a record.
AMDMSM_DEV void frd_root_power(F& x, const uint32_t* tw, size_t i, size_t half) {
    const bool neg = i >= half;
    rec_load(x, tw, neg ? i - half : i);
    fp_cneg(x, x, neg);
}
template <bool UNIT>
__global__ void __launch_bounds__(TPB) k_frd_lagrange(const frd_lagrange a) {
    const size_t O = (size_t)1 << a.log_o, half = O >> 1;
    const size_t B = a.step ? (size_t)1 << a.log_b : 0, kmask = a.step ? (B >> a.log_s) - 1 : 0;
    F t, tail, one;
    rec_copy(t, a.t);
    rec_copy(tail, a.tail);
    fp_set_one(one);
    for (size_t j = (size_t)blockIdx.x * TPB + threadIdx.x; j < a.m; j += (size_t)gridDim.x * TPB) {
        const size_t e = !a.step ? j : (j < B ? 2 * j : 1 + ((j - B) << (a.log_o - a.log_s)));
        F x;
        if constexpr (UNIT) {
            frd_root_power(x, a.tw, e, half);
            const bool hit = fp_eq(x, t);
            fp_set_zero(x);
            rec_store(a.out, j, hit ? tail : x);
        } else {
            frd_root_power(x, a.tw, (O - e) & (O - 1), half);   // 1 / x_j
            F f = tail;
            if (j < B) rec_load(f, a.kden, j & kmask);
            fp_mul(x, x, t);
            fp_sub(x, x, one);
            fp_mul(x, x, f);
            rec_store(a.out, j, x);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void l_domain_sweep(hipStream_t st, const frd_sweep& a) {
    const uint32_t per = (uint32_t)(TPB >> a.log_w) * a.iters;
    const dim3 grid(((a.rows + per - 1) / per) << (a.log_s - a.log_w));   // at most B / 1024 = 2^17 workgroups
    if (a.mode == FRD_FOLD) hipLaunchKernelGGL(k_frd_sweep<FRD_FOLD>, grid, dim3(TPB), 0, st, a);
    else if (a.mode == FRD_MERGE) hipLaunchKernelGGL(k_frd_sweep<FRD_MERGE>, grid, dim3(TPB), 0, st, a);
    else hipLaunchKernelGGL(k_frd_sweep<FRD_REDUCE>, grid, dim3(TPB), 0, st, a);
}
void l_domain_combine(hipStream_t st, const frd_combine& a) {
    const size_t S = (size_t)1 << a.log_s;
    hipLaunchKernelGGL(k_frd_combine, dim3((unsigned)((S + TPB - 1) / TPB)), dim3(TPB), 0, st, a);
}
void l_domain_den(hipStream_t st, size_t n, uint32_t* d_den, const uint32_t* c) {
    fr_rec_arg cc = {};
    for (int w = 0; w < N; ++w) cc.v[w] = c[w];
    hipLaunchKernelGGL(k_frd_den, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, n, d_den, cc);
}
void l_domain_divide(hipStream_t st, size_t m, size_t B, size_t K, const uint32_t* d_in, const uint32_t* d_inv, const uint32_t* tail,
                     uint32_t* d_out) {
    fr_rec_arg tl = {};
    for (int w = 0; w < N; ++w) tl.v[w] = tail[w];
    const size_t blocks = (m + TPB - 1) / TPB;
    hipLaunchKernelGGL(k_frd_divide, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(TPB), 0, st, m, B, K ? K - 1 : 0, d_in,
                       d_inv, tl, d_out);
}
void l_domain_lagrange(hipStream_t st, const frd_lagrange& a) {
    const size_t blocks = (a.m + TPB - 1) / TPB;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (a.unit) hipLaunchKernelGGL(k_frd_lagrange<true>, grid, dim3(TPB), 0, st, a);
    else hipLaunchKernelGGL(k_frd_lagrange<false>, grid, dim3(TPB), 0, st, a);
}
