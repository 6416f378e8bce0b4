// Scans and batch inversion over a vector of Fr records (amdmsm_fr_scan, amdmsm_fr_batch_invert): the first-order
// recurrence y_i = a_i y_(i-1) + b_i as a scan over the maps y -> a y + b, which compose associatively --
// (a2, b2) o (a1, b1) = (a2 a1, a2 b1 + b2) -- and Montgomery's batch inversion on the same skeleton.  Included by
// fr_ntt.hip inside its anonymous namespace, once per scalar field; DESIGN section 20, indices in fr_scan_layout.h.
//
// No kernel waits for another workgroup.  Three launches in stream order:
//   reduce   a workgroup composes the maps of its tile -- 256 lanes with E consecutive positions each, staged through
//            the LDS tile of the transform so that the global loads stay coalesced -- and leaves the tile's (A, B)
//   spine    one workgroup walks the aggregates, a step at a time -- every lane a few consecutive ones -- with a serial
//            carry between steps, leaves every tile's incoming value and writes the total
//   apply    a workgroup reads its tile again, finds every lane's incoming value from the tile's and stores the results
// HA / HB say whether a and b exist: A is not carried when every a_i is 1, B is neither carried nor stored without b.
// Every index comes from n and the launch geometry, none from a record: a record that is no field element changes
// values, never an address.

constexpr uint32_t FRS_E = FRS_PER_LANE_MAX;
static_assert(FRS_LANES == TPB && (1u << FRS_TILE_MAX) <= E, "a tile of the scan fits the LDS tile of the transform");
static_assert(FRS_SLOT_AUX < E, "the block scan's slots lie inside the LDS tile");

AMDMSM_DEV void frs_one(F& r) { fp_set_one(r); }

// (A, B) = (A, B) o (A1, B1): the map (A1, B1) first
template <bool HA, bool HB>
AMDMSM_DEV void frs_after(F& A, F& B, const F& A1, const F& B1) {
    if constexpr (HB) {
        if constexpr (HA) {
            F t;
            fp_mul(t, A, B1);
            fp_add(B, B, t);
        } else {
            fp_add(B, B, B1);
        }
    }
    if constexpr (HA) fp_mul(A, A, A1);
}
// y = A y + B
template <bool HA, bool HB>
AMDMSM_DEV void frs_eval(F& y, const F& A, const F& B) {
    if constexpr (HA) fp_mul(y, y, A);
    if constexpr (HB) fp_add(y, y, B);
}
template <bool HA, bool HB>
AMDMSM_DEV void frs_identity(F& A, F& B) {
    if constexpr (HA) frs_one(A);
    if constexpr (HB) fp_set_zero(B);
}
AMDMSM_DEV void frs_shfl_up(F& r, const F& a, int d) {
#pragma unroll
    for (int w = 0; w < N; ++w) r.v[w] = __shfl_up(a.v[w], d);
}

// The 256 lanes' maps (A, B), lane 0 first, become each lane's exclusive prefix -- the composition of the lanes before
// it -- and (TA, TB) the composition of all.  The maps go through the LDS tile, whose records the caller holds in
// registers by now: the first wave folds four neighbours to a lane, scans the 64 results with shuffles on the record
// words and writes the 256 prefixes back, which costs a dozen dependent products of one wave where a shuffle scan in
// every wave costs six in each of the four.  REV: lane 255 first (a suffix).
template <bool HA, bool HB, bool REV>
AMDMSM_DEV void frs_block_scan(uint2 (*tile)[E], uint32_t tid, F& A, F& B, F& TA, F& TB) {
    const uint32_t me = REV ? FRS_LANES - 1 - tid : tid;
    __syncthreads();   // the tile is free
    if constexpr (HA) tile_put(tile, FRS_SLOT_A + me, A);
    if constexpr (HB) tile_put(tile, FRS_SLOT_B + me, B);
    __syncthreads();
    if (tid < 64) {
        F pa[4], pb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (HA) tile_get(pa[q], tile, FRS_SLOT_A + 4 * tid + q);
            if constexpr (HB) tile_get(pb[q], tile, FRS_SLOT_B + 4 * tid + q);
            if (q) frs_after<HA, HB>(pa[q], pb[q], pa[q - 1], pb[q - 1]);
        }
        F ia = pa[3], ib = pb[3];   // inclusive over the wave
#pragma unroll 1
        for (int d = 1; d < 64; d <<= 1) {
            F ua, ub;
            if constexpr (HA) frs_shfl_up(ua, ia, d);
            if constexpr (HB) frs_shfl_up(ub, ib, d);
            if (tid >= (uint32_t)d) frs_after<HA, HB>(ia, ib, ua, ub);
        }
        F xa, xb;                   // exclusive: what the lane before has
        if constexpr (HA) frs_shfl_up(xa, ia, 1);
        if constexpr (HB) frs_shfl_up(xb, ib, 1);
        if (tid == 0) frs_identity<HA, HB>(xa, xb);
        if (tid == 63) {
            if constexpr (HA) tile_put(tile, FRS_SLOT_TOTAL, ia);
            if constexpr (HB) tile_put(tile, FRS_SLOT_TOTAL + 1, ib);
        }
        if constexpr (HA) tile_put(tile, FRS_SLOT_A + 4 * tid, xa);
        if constexpr (HB) tile_put(tile, FRS_SLOT_B + 4 * tid, xb);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            frs_after<HA, HB>(pa[q], pb[q], xa, xb);
            if constexpr (HA) tile_put(tile, FRS_SLOT_A + 4 * tid + q + 1, pa[q]);
            if constexpr (HB) tile_put(tile, FRS_SLOT_B + 4 * tid + q + 1, pb[q]);
        }
    }
    __syncthreads();
    if constexpr (HA) {
        tile_get(A, tile, FRS_SLOT_A + me);
        tile_get(TA, tile, FRS_SLOT_TOTAL);
    }
    if constexpr (HB) {
        tile_get(B, tile, FRS_SLOT_B + me);
        tile_get(TB, tile, FRS_SLOT_TOTAL + 1);
    }
    __syncthreads();
}

// The tile's records of one vector into the lanes' registers: v[k] = the record at the lane's k-th position, `pad`
// beyond n.  Coalesced loads into the LDS tile, then every lane takes its E neighbours
AMDMSM_DEV void frs_load_tile(uint2 (*tile)[E], const frs_args& a, const uint32_t* src, uint32_t tid, F (&v)[FRS_E], const F& pad) {
    const uint32_t T = 1u << a.tile_log2, per = T >> FRS_LANES_LOG2;
    const size_t base = frs_tile_base(blockIdx.x, a.tile_log2);
    __syncthreads();   // the tile is free
    for (uint32_t e = tid; e < T; e += TPB) {
        const size_t p = base + e;
        F x = pad;
        if (p < a.n) {
            rec_load(x, src, frs_record(a.n, a.reverse != 0, p));
            if (a.plain) fp_to_mont(x, x);
        }
        tile_put(tile, e, x);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < FRS_E; ++k)
        if (k < per) tile_get(v[k], tile, frs_lane_slot(tid, k, a.tile_log2));
}
// the lanes' results to the caller's vector, through the tile again
AMDMSM_DEV void frs_store_tile(uint2 (*tile)[E], const frs_args& a, uint32_t tid, const F (&v)[FRS_E]) {
    const uint32_t T = 1u << a.tile_log2, per = T >> FRS_LANES_LOG2;
    const size_t base = frs_tile_base(blockIdx.x, a.tile_log2);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < FRS_E; ++k)
        if (k < per) tile_put(tile, frs_lane_slot(tid, k, a.tile_log2), v[k]);
    __syncthreads();
    for (uint32_t e = tid; e < T; e += TPB) {
        const size_t p = base + e;
        if (p >= a.n) continue;
        F x;
        tile_get(x, tile, e);
        if (a.plain) fp_from_mont(x, x);
        rec_store(a.out, frs_record(a.n, a.reverse != 0, p), x);
    }
}

// the a and b of a tile in registers: identity maps beyond n
template <bool HA, bool HB>
AMDMSM_DEV void frs_load_maps(uint2 (*tile)[E], const frs_args& a, uint32_t tid, F (&av)[FRS_E], F (&bv)[FRS_E]) {
    if constexpr (HA) {
        F one;
        frs_one(one);
        if (a.has_a == 1) {
            frs_load_tile(tile, a, a.a, tid, av, one);
        } else {
            F c;
            rec_copy(c, a.a_const);
            const size_t first = frs_tile_base(blockIdx.x, a.tile_log2) + frs_lane_slot(tid, 0, a.tile_log2);
#pragma unroll
            for (uint32_t k = 0; k < FRS_E; ++k) av[k] = first + k < a.n ? c : one;
        }
    }
    if constexpr (HB) {
        F zero;
        fp_set_zero(zero);
        frs_load_tile(tile, a, a.b, tid, bv, zero);
    }
}
// the composition of a lane's maps, the first position first
template <bool HA, bool HB>
AMDMSM_DEV void frs_fold_lane(const frs_args& a, const F (&av)[FRS_E], const F (&bv)[FRS_E], F& A, F& B) {
    const uint32_t per = 1u << (a.tile_log2 - FRS_LANES_LOG2);
    if constexpr (HA) A = av[0];
    if constexpr (HB) B = bv[0];
#pragma unroll
    for (uint32_t k = 1; k < FRS_E; ++k) {
        if (k < per) {
            F ka, kb;
            if constexpr (HA) ka = av[k];
            if constexpr (HB) kb = bv[k];
            frs_after<HA, HB>(ka, kb, A, B);
            if constexpr (HA) A = ka;
            if constexpr (HB) B = kb;
        }
    }
}

// ---- reduce ----------------------------------------------------------------------------------------------------------
template <bool HA, bool HB>
__global__ void __launch_bounds__(TPB) k_frs_reduce(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    F av[FRS_E], bv[FRS_E], A, B, TA, TB;
    frs_load_maps<HA, HB>(tile, a, tid, av, bv);
    frs_fold_lane<HA, HB>(a, av, bv, A, B);
    frs_block_scan<HA, HB, false>(tile, tid, A, B, TA, TB);
    if (tid == 0) {
        if constexpr (HA) rec_store(a.ws_a, blockIdx.x, TA);
        if constexpr (HB) rec_store(a.ws_b, blockIdx.x, TB);
    }
}

// ---- spine -----------------------------------------------------------------------------------------------------------
// One workgroup; y, the carry, is the same in every lane.  Writes ws_in[t] = the value that enters tile t, and the total.
template <bool HA, bool HB>
__global__ void __launch_bounds__(TPB) k_frs_spine(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    const uint32_t G = frs_spine_per_lane(a.tile_log2, a.tiles);
    const size_t steps = frs_spine_steps(a.tiles, G);
    F y;
    rec_copy(y, a.init);
#pragma unroll 1
    for (size_t s = 0; s < steps; ++s) {
        F A, B, TA, TB;
        frs_identity<HA, HB>(A, B);
#pragma unroll 1
        for (uint32_t g = 0; g < G; ++g) {   // the lane's aggregates, the first one first
            const size_t t = frs_spine_tile(a.tiles, G, s, tid, g, false);
            if (t >= a.tiles) break;
            F ta, tb;
            if constexpr (HA) rec_load(ta, a.ws_a, t);
            if constexpr (HB) rec_load(tb, a.ws_b, t);
            frs_after<HA, HB>(ta, tb, A, B);
            if constexpr (HA) A = ta;
            if constexpr (HB) B = tb;
        }
        frs_block_scan<HA, HB, false>(tile, tid, A, B, TA, TB);
        F in = y;
        frs_eval<HA, HB>(in, A, B);   // what enters the lane's first tile
#pragma unroll 1
        for (uint32_t g = 0; g < G; ++g) {
            const size_t t = frs_spine_tile(a.tiles, G, s, tid, g, false);
            if (t >= a.tiles) break;
            rec_store(a.ws_in, t, in);
            F ta, tb;
            if constexpr (HA) rec_load(ta, a.ws_a, t);
            if constexpr (HB) rec_load(tb, a.ws_b, t);
            frs_eval<HA, HB>(in, ta, tb);
        }
        frs_eval<HA, HB>(y, TA, TB);
    }
    if (tid == 0 && a.total) {
        if (a.plain) fp_from_mont(y, y);
        rec_store(a.total, 0, y);
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------
template <bool HA, bool HB>
__global__ void __launch_bounds__(TPB) k_frs_apply(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = 1u << (a.tile_log2 - FRS_LANES_LOG2);
    F av[FRS_E], bv[FRS_E], A, B, TA, TB, y;
    frs_load_maps<HA, HB>(tile, a, tid, av, bv);
    frs_fold_lane<HA, HB>(a, av, bv, A, B);
    frs_block_scan<HA, HB, false>(tile, tid, A, B, TA, TB);
    rec_load(y, a.ws_in, blockIdx.x);
    frs_eval<HA, HB>(y, A, B);   // what enters the lane
    F res[FRS_E];
#pragma unroll
    for (uint32_t k = 0; k < FRS_E; ++k) {
        if (k < per) {
            if (a.exclusive) res[k] = y;
            frs_eval<HA, HB>(y, av[k], bv[k]);
            if (!a.exclusive) res[k] = y;
        }
    }
    frs_store_tile(tile, a, tid, res);
}

// ---- batch inversion -------------------------------------------------------------------------------------------------
// The same skeleton on products, a zero record taken as 1: reduce leaves the tiles' products (and zero counts), the
// spine inverts the product of all of them -- once, in one lane -- and leaves every tile the inverse of its own product,
// apply does the same among the lanes of a tile and ends with Montgomery's back-sweep over a lane's records.
AMDMSM_DEV uint32_t frs_zero_to_one(const frs_args& a, uint32_t per, F (&x)[FRS_E]) {
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t k = 0; k < FRS_E; ++k) {
        if (k < per && fp_is_zero(x[k])) {
            mask |= 1u << k;
            frs_one(x[k]);
        }
    }
    return mask;
}

__global__ void __launch_bounds__(TPB) k_frs_inv_reduce(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    __shared__ uint32_t zeros;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = 1u << (a.tile_log2 - FRS_LANES_LOG2);
    if (tid == 0) zeros = 0;
    F x[FRS_E], none[FRS_E], one, A, B, TA, TB;
    frs_one(one);
    frs_load_tile(tile, a, a.a, tid, x, one);
    const uint32_t mask = frs_zero_to_one(a, per, x);
    if (mask) atomicAdd(&zeros, (uint32_t)__popc(mask));
    frs_fold_lane<true, false>(a, x, none, A, B);
    frs_block_scan<true, false, false>(tile, tid, A, B, TA, TB);   // its barriers also stand behind the count
    if (tid == 0) {
        rec_store(a.ws_a, blockIdx.x, TA);
        a.ws_cnt[blockIdx.x] = zeros;
    }
}

// ws_in[t] = 1 / (product of tile t) = (1 / product of all) * (product of the tiles before t) * (product of those behind)
__global__ void __launch_bounds__(TPB) k_frs_inv_spine(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    __shared__ unsigned long long zeros;
    const uint32_t tid = threadIdx.x;
    const uint32_t G = frs_spine_per_lane(a.tile_log2, a.tiles);
    const size_t steps = frs_spine_steps(a.tiles, G);
    if (tid == 0) zeros = 0;
    unsigned long long mine = 0;
    F y, B, TB;
    frs_one(y);
    // sweep 0: ws_in[t] = the product of the tiles before t, y = the product of all; then the one inversion of the call;
    // sweep 1, from the last tile down: ws_in[t] *= (1 / product of all) * (the product of the tiles behind t)
#pragma unroll 1
    for (int sweep = 0; sweep < 2; ++sweep) {
        const bool back = sweep == 1;
#pragma unroll 1
        for (size_t s = 0; s < steps; ++s) {
            F A, TA;
            frs_one(A);
#pragma unroll 1
            for (uint32_t g = 0; g < G; ++g) {
                const size_t t = frs_spine_tile(a.tiles, G, s, tid, g, back);
                if (t >= a.tiles) break;
                F ta;
                rec_load(ta, a.ws_a, t);
                fp_mul(A, A, ta);
                if (!back) mine += a.ws_cnt[t];
            }
            frs_block_scan<true, false, false>(tile, tid, A, B, TA, TB);
            fp_mul(A, A, y);
#pragma unroll 1
            for (uint32_t g = 0; g < G; ++g) {
                const size_t t = frs_spine_tile(a.tiles, G, s, tid, g, back);
                if (t >= a.tiles) break;
                F ta, v = A;
                if (back) {
                    rec_load(ta, a.ws_in, t);
                    fp_mul(v, v, ta);
                }
                rec_store(a.ws_in, t, v);
                rec_load(ta, a.ws_a, t);
                fp_mul(A, A, ta);
            }
            fp_mul(y, y, TA);
        }
        if (back) break;
        if (mine) atomicAdd(&zeros, mine);
        if (tid == 0) {   // one lane
            F inv;
            fp_inv(inv, y);
            tile_put(tile, FRS_SLOT_AUX, inv);
        }
        __syncthreads();
        tile_get(y, tile, FRS_SLOT_AUX);
        if (tid == 0 && a.zero_count) *a.zero_count = zeros;
    }
}

__global__ void __launch_bounds__(TPB) k_frs_inv_apply(const frs_args a) {
    __shared__ uint2 tile[N / 2][E];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = 1u << (a.tile_log2 - FRS_LANES_LOG2);
    F x[FRS_E], c[FRS_E], one, B, TA, TB;
    frs_one(one);
    frs_load_tile(tile, a, a.a, tid, x, one);
    const uint32_t mask = frs_zero_to_one(a, per, x);
    // c[k] = x[0] .. x[k]
    c[0] = x[0];
#pragma unroll
    for (uint32_t k = 1; k < FRS_E; ++k)
        if (k < per) fp_mul(c[k], c[k - 1], x[k]);
    F lane = c[0];
#pragma unroll
    for (uint32_t k = 1; k < FRS_E; ++k)
        if (k < per) lane = c[k];
    F before = lane, behind = lane, inv;
    frs_block_scan<true, false, false>(tile, tid, before, B, TA, TB);
    frs_block_scan<true, false, true>(tile, tid, behind, B, TA, TB);
    rec_load(inv, a.ws_in, blockIdx.x);
    fp_mul(inv, inv, before);
    fp_mul(inv, inv, behind);   // 1 / (the lane's product)
    // back-sweep: 1 / x[k] = inv * c[k - 1], then inv loses x[k]
    F res[FRS_E];
#pragma unroll
    for (int k = FRS_E - 1; k >= 0; --k) {
        if ((uint32_t)k < per) {
            if (k) fp_mul(res[k], inv, c[k - 1]);
            else res[k] = inv;
            if (k) fp_mul(inv, inv, x[k]);
            if ((mask >> k) & 1u) fp_set_zero(res[k]);
        }
    }
    frs_store_tile(tile, a, tid, res);
}

// ---- AMDMSM_FR_SCAN_NAIVE=1: one lane walks the recurrence; the inversion is Montgomery's trick as libff's
// batch_invert writes it, the running products in the workspace --------------------------------------------------------
__global__ void __launch_bounds__(64) k_frs_naive(const frs_args a) {
    if (blockIdx.x || threadIdx.x) return;
    const bool rev = a.reverse != 0;
    F one;
    frs_one(one);
    if (a.invert) {
        F acc = one;
        unsigned long long zeros = 0;
        for (size_t p = 0; p < a.n; ++p) {
            F x;
            rec_load(x, a.a, p);
            if (a.plain) fp_to_mont(x, x);
            if (fp_is_zero(x)) {
                x = one;
                ++zeros;
            }
            rec_store(a.ws_a, p, acc);
            fp_mul(acc, acc, x);
        }
        F inv;
        fp_inv(inv, acc);
        for (size_t p = a.n; p-- > 0;) {
            F x, prod, r;
            rec_load(x, a.a, p);
            if (a.plain) fp_to_mont(x, x);
            const bool zero = fp_is_zero(x);
            if (zero) x = one;
            rec_load(prod, a.ws_a, p);
            fp_mul(r, inv, prod);
            fp_mul(inv, inv, x);
            if (zero) fp_set_zero(r);
            if (a.plain) fp_from_mont(r, r);
            rec_store(a.out, p, r);
        }
        if (a.zero_count) *a.zero_count = zeros;
        return;
    }
    F y, c;
    rec_copy(y, a.init);
    rec_copy(c, a.a_const);
    for (size_t p = 0; p < a.n; ++p) {
        const size_t i = frs_record(a.n, rev, p);
        F x, b, o;
        if (a.has_a == 1) {
            rec_load(x, a.a, i);
            if (a.plain) fp_to_mont(x, x);
        } else {
            x = c;
        }
        if (a.has_b) {
            rec_load(b, a.b, i);
            if (a.plain) fp_to_mont(b, b);
        }
        o = y;
        if (a.has_a) fp_mul(y, y, x);
        if (a.has_b) fp_add(y, y, b);
        if (!a.exclusive) o = y;
        if (a.plain) fp_from_mont(o, o);
        rec_store(a.out, i, o);
    }
    if (a.total) {
        if (a.plain) fp_from_mont(y, y);
        rec_store(a.total, 0, y);
    }
}

template <bool HA, bool HB>
void frs_launch(hipStream_t st, const frs_args& a) {
    if (a.tiles) hipLaunchKernelGGL((k_frs_reduce<HA, HB>), dim3(a.tiles), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL((k_frs_spine<HA, HB>), dim3(1), dim3(TPB), 0, st, a);
    if (a.tiles) hipLaunchKernelGGL((k_frs_apply<HA, HB>), dim3(a.tiles), dim3(TPB), 0, st, a);
}
void l_scan(hipStream_t st, const frs_args& a) {
    if (a.invert) {
        if (a.tiles) hipLaunchKernelGGL(k_frs_inv_reduce, dim3(a.tiles), dim3(TPB), 0, st, a);
        hipLaunchKernelGGL(k_frs_inv_spine, dim3(1), dim3(TPB), 0, st, a);
        if (a.tiles) hipLaunchKernelGGL(k_frs_inv_apply, dim3(a.tiles), dim3(TPB), 0, st, a);
    } else if (a.has_a && a.has_b) {
        frs_launch<true, true>(st, a);
    } else if (a.has_a) {
        frs_launch<true, false>(st, a);
    } else {
        frs_launch<false, true>(st, a);
    }
}
void l_scan_naive(hipStream_t st, const frs_args& a) { hipLaunchKernelGGL(k_frs_naive, dim3(1), dim3(64), 0, st, a); }
