// Sparse matrix times point vector (amdmsm_group_matrix_apply): the kernels over the resident form of fr_matrix_layout.h,
// the one amdmsm_fr_matrix_load keeps in HBM for k_frm_apply.  Included by msm_group.hip inside its anonymous namespace,
// once per group; DESIGN section 28.
//
// A general entry's product coeff * P[col] is made before the accumulation, by the ladder of scalar_mul_vec over the
// gathered points, and normalised to a compact affine record: the accumulation then adds affine records only -- P[col],
// -P[col] or T[rank] -- with the complete xyzz_madd.  Every address comes from the arrays the load built (columns <
// n_cols <= n_points, rows < n_rows, partials < n_partials, ranks below the count of general entries) and none from
// point data.

// the rank of a general lane among the job's general entries in word order, as k_frm_apply takes it
AMDMSM_DEV uint32_t gm_rank_below(uint64_t gen) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(gen >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)gen, 0u));
}

// gathered[rank - first_rank] = P[col] for every general entry of the jobs job0 .. job0 + n_jobs - 1, one wave per job
__global__ void __launch_bounds__(TPB) k_gm_gather(const gm_args a) {
    const uint32_t lane = threadIdx.x & (FRM_LANES - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (TPB / FRM_LANES) + threadIdx.x / FRM_LANES);
    if (wave >= a.n_jobs) return;
    const frm_desc d = a.desc[a.job0 + wave];
    const uint32_t* words = a.words + (size_t)d.base64 * FRM_LANES + lane;
    uint32_t rank0 = d.gen_base - a.first_rank;
    for (uint32_t j = 0; j < d.steps; ++j) {
        const uint32_t w = words[(size_t)j * FRM_LANES];
        const bool is_gen = (w >> FRM_COL_BITS) == FRM_GEN;
        const uint64_t gen = __ballot(is_gen);
        if (is_gen) {
            Aff<E> p;
            load_aff(p, a.points + (size_t)(w & FRM_COL_MASK) * AFFW);
            store_aff(a.prod + ((size_t)rank0 + gm_rank_below(gen)) * AFFW, p);
        }
        rank0 += (uint32_t)__popcll(gen);
    }
}

template <class T> AMDMSM_DEV void xyzz_shfl_xor(Xyzz<T>& r, const Xyzz<T>& p, int mask) {
    el_shfl_xor(r.x, p.x, mask);
    el_shfl_xor(r.y, p.y, mask);
    el_shfl_xor(r.zz, p.zz, mask);
    el_shfl_xor(r.zzz, p.zzz, mask);
}

// One wave per job, the walk of k_frm_apply: lane l reads word (base64 + j) * 64 + l in step j and adds its point to the
// lane's accumulator.  A lanes job writes one row per lane; a row or part job folds the 64 sums by a butterfly of
// complete additions (equal sums double, opposite sums cancel) and lane 0 writes the row, or the partial sum as an
// (X, Y, ZZ, ZZZ) record for k_gm_combine.
__global__ void __launch_bounds__(TPB) k_gm_apply(const gm_args a) {
    const uint32_t lane = threadIdx.x & (FRM_LANES - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (TPB / FRM_LANES) + threadIdx.x / FRM_LANES);
    if (wave >= a.n_jobs) return;
    const frm_desc d = a.desc[a.job0 + wave];
    const uint32_t mode = d.dest >> FRM_MODE_SHIFT, dest = d.dest & FRM_DEST_MASK;
    const uint32_t* words = a.words + (size_t)d.base64 * FRM_LANES + lane;
    Xyzz<E> acc;
    xyzz_set_inf(acc);
    Aff<E> e;
    uint32_t rank0 = d.gen_base - a.first_rank;
#pragma unroll 1
    for (uint32_t j = 0; j < d.steps; ++j) {
        const uint32_t w = words[(size_t)j * FRM_LANES];
        const uint32_t cls = w >> FRM_COL_BITS;
        const uint64_t gen = __ballot(cls == FRM_GEN);
        if (cls != FRM_PAD) {
            const uint32_t* src = cls == FRM_GEN ? a.prod + ((size_t)rank0 + gm_rank_below(gen)) * AFFW
                                                 : a.points + (size_t)(w & FRM_COL_MASK) * AFFW;
            load_aff(e, src);
            el_cneg(e.y, e.y, cls == FRM_MINUS);
            xyzz_madd(acc, e);
        }
        rank0 += (uint32_t)__popcll(gen);
    }
    Jac<E> res;
    if (mode == FRM_MODE_LANES) {
        const uint32_t row = a.lane_rows[(size_t)dest * FRM_LANES + lane];
        if (row != FRM_NO_ROW) {
            xyzz_to_jac(res, acc);
            store_out(a.out + (size_t)row * XYZW, res, a.form);
        }
        return;
    }
#pragma unroll 1
    for (int s = FRM_LANES / 2; s; s >>= 1) {
        Xyzz<E> other;
        xyzz_shfl_xor(other, acc, s);
        xyzz_add(acc, acc, other);
    }
    if (lane != 0) return;
    if (mode == FRM_MODE_PART) {
        store_xyzz(a.partial + (size_t)dest * ZZW, acc);
    } else {
        xyzz_to_jac(res, acc);
        store_out(a.out + (size_t)dest * XYZW, res, a.form);
    }
}

// out[row] = the sum of the row's partials in order, one lane per split row
__global__ void __launch_bounds__(TPB) k_gm_combine(const frm_comb* __restrict__ comb, uint32_t n_comb,
                                                    const uint32_t* __restrict__ partial, int form, uint32_t* __restrict__ out) {
    const size_t i = gtid();
    if (i >= n_comb) return;
    const frm_comb c = comb[i];
    Xyzz<E> acc, x;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (uint32_t p = 0; p < c.count; ++p) {
        load_xyzz(x, partial + ((size_t)c.first + p) * ZZW);
        xyzz_add(acc, acc, x);
    }
    Jac<E> res;
    xyzz_to_jac(res, acc);
    store_out(out + (size_t)c.row * XYZW, res, form);
}

void l_gm_gather(hipStream_t st, const gm_args& a) {
    if (!a.n_jobs) return;
    hipLaunchKernelGGL(k_gm_gather, dim3(blocks_for((size_t)a.n_jobs * FRM_LANES)), dim3(TPB), 0, st, a);
}
void l_gm_apply(hipStream_t st, const gm_args& a) {
    if (!a.n_jobs) return;
    hipLaunchKernelGGL(k_gm_apply, dim3(blocks_for((size_t)a.n_jobs * FRM_LANES)), dim3(TPB), 0, st, a);
}
void l_gm_combine(hipStream_t st, const frm_comb* comb, uint32_t n_comb, const uint32_t* partial, int form, uint32_t* out) {
    if (!n_comb) return;
    hipLaunchKernelGGL(k_gm_combine, dim3(blocks_for(n_comb)), dim3(TPB), 0, st, comb, n_comb, partial, form, out);
}
