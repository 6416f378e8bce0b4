// Host side of the amdmsm C ABI (include/amdmsm.h): context, workspace, the MSM
// pipeline schedule and the host-buffer entry points.  All arithmetic on vectors happens in
// the kernels of msm_group.hip and fr_ntt.hip; there is no CPU arithmetic path in this library
// (the scalar FFT's host side squares its handful of parameters, nothing more).
#include "../../include/amdmsm.h"
#include "engine_internal.h"
#include "group_vtable.h"
#include "fr_vtable.h"
#include "write_plan.h"

#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace amdmsm;

// One workspace "slot" per MSM in flight.  With pipeline depth > 1 consecutive
// amdmsm_msm_device calls take the slots round-robin, so calls issued on different streams
// may overlap on the device (the small-grid tail of one MSM under the bulk kernels of the
// next); a slot is reused only after the call that last used it has finished (event wait).
constexpr int MAX_SLOTS = 4;
// Window groups of one MSM (experimental, off by default: AMDMSM_WINDOW_GROUPS=2..4): the windows
// are accumulated group by group on the caller's stream, highest first; the tail of a finished
// group (bucket fix-up, reduction, its share of the Horner chain) runs on a side stream under
// the accumulation of the next group.  Measured gain is only ~3% at 2^20..2^22 and ~1% at 2^26:
// the tail kernels are short on parallelism, not on issue slots, and slow down 2-3x when they
// share SIMDs with k_accumulate.
constexpr int MAX_GROUPS = 4;
struct ws_slot {
    void *ws = nullptr;
    size_t ws_bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
    hipStream_t side[MAX_GROUPS - 1] = {};
    hipEvent_t acc_done[MAX_GROUPS - 1] = {}, tail_done[MAX_GROUPS - 1] = {};
    long long last_ticket = -1;   // timing ticket of the call that last used the slot
    bool ev_valid = false;
    hipEvent_t ov_in = nullptr, ov_acc = nullptr, ov_tail = nullptr;   // overlap mode (see amdmsm_ctx::bulk_stream)
};

// grow-only device buffer kept by the context between calls (host-buffer entry points)
struct grow_buf {
    void *p = nullptr;
    size_t bytes = 0;
};

// Base vector imported once and kept in HBM as compact affine records (amdmsm_register_bases):
// the proving key of a prover that calls multi_exp with the same bases proof after proof.
// Host-buffer calls whose base range lies inside [host, host + n*stride) use the resident copy.
struct base_entry {
    uint64_t id = 0;
    int curve = 0, group = 0, form = 0;
    const char *host = nullptr;
    size_t n = 0, stride = 0;
    void *d_aff = nullptr;
    void *d_endo = nullptr;   // phi(P) records of the whole vector (endomorphism split), built at first use
    bool automatic = false;   // created by AMDMSM_BASE_CACHE, evictable
    bool pinned = false;      // resolved by the batch call that is running: not evictable until it returns
    uint64_t last_use = 0;
    size_t aff_bytes = 0;     // bytes of one compact affine record of this entry's group
    // HBM held by the entry: the affine copy and, once built, the phi(P) records
    size_t bytes() const { return n * aff_bytes * (d_endo ? 2 : 1); }
};

// fixed-base exponentiation state kept between amdmsm_batch_exp calls: buffers and the resident window table
struct fb_state {
    grow_buf small, table, table_aff, out;
    bool valid = false;
    int curve = 0, group = 0;
    size_t scalar_size = 0, window = 0;
    unsigned char g[3 * 24 * 2 * 4] = {};   // the generator the resident table was built from
    // amdmsm_batch_exp_device runs on the caller's stream and does not wait: `used` is recorded behind the last such call
    // -- the table it built or read, the coefficient slot of `small` -- and every later call of either entry makes its own
    // stream wait for it, as a workspace slot's `done` does.  h_up: UP_BLOCKS pinned copies of (g, coeff), taken in
    // turn: the entry copies its host arguments there before it returns; uploaded[b], behind the copy out of block b,
    // is what the call that takes block b next waits for on the host -- UP_BLOCKS calls later, not the next one.
    static constexpr unsigned UP_BLOCKS = 4;
    hipEvent_t used = nullptr, uploaded[UP_BLOCKS] = {};
    bool used_valid = false, uploaded_valid[UP_BLOCKS] = {};
    unsigned up_next = 0;
    void *h_up = nullptr;
};

// staging of the streaming entries (multi_exp_stream*), kept between calls
struct stream_state {
    static constexpr int NB = 2;
    void *h_stage[NB] = {};
    size_t h_bytes[NB] = {};
    grow_buf d_raw[NB], d_aff[NB], d_sc[NB], partials, status;
    hipStream_t streams[NB] = {};
};

// the n / 2 powers of omega a scalar FFT has used, kept for the next one over the same domain (amdmsm_fr_fft)
struct fr_tw_entry {
    int curve = -1;
    size_t n = 0;
    uint32_t omega[amdmsm::FR_MAX_WORDS] = {};
    grow_buf buf;
    hipEvent_t ev = nullptr;   // behind the last call that built or read buf
    uint64_t last_use = 0;
};

// A sparse matrix over Fr kept in HBM (amdmsm_fr_matrix_load): the resident form of fr_matrix_layout.h, or with
// AMDMSM_FR_MATRIX_NAIVE=1 the caller's CSR arrays.  Owned by the context; known to callers by its id.
struct fr_matrix {
    uint64_t id = 0;
    int curve = 0;
    size_t n_rows = 0, n_cols = 0, kept = 0;     // kept: entries an apply reads
    bool naive = false;
    void *words = nullptr, *coef = nullptr, *desc = nullptr, *lane_rows = nullptr, *comb = nullptr;   // resident form
    void *offsets = nullptr, *cols = nullptr;                                                         // naive: with coef
    uint32_t n_desc = 0, n_comb = 0, n_partials = 0;
    // host copy of every job's gen_base and, behind the last, the count of general entries: where
    // amdmsm_group_matrix_apply cuts its chunks
    std::vector<uint32_t> job_gen;
    // behind the last apply on every stream that has used the handle: what amdmsm_fr_matrix_free waits for
    std::vector<std::pair<hipStream_t, hipEvent_t>> users;
};

struct amdmsm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    ws_slot slots[MAX_SLOTS];
    int depth = 1;
    unsigned next = 0;
    int last_slot = 0;
    bool timing = false;
    hipEvent_t ev[AMDMSM_MAX_PHASES + 1] = {};   // probes
    // phase events of the last TIMING_RING timed MSMs, indexed by ticket % TIMING_RING: a caller
    // can enqueue MSM after MSM without synchronising and read every call's phase times afterwards
    hipEvent_t ring[64][6] = {};
    uint64_t ticket = 0;      // tickets handed out so far (the last call's ticket is ticket - 1)
    void *chunk_partials = nullptr;               // a few points, for calls split into several MSMs
    // host-buffer entry points: staging in HBM reused across calls, a second stream that brings
    // the bases in while the scalars are already being sorted, and the resident base vectors
    grow_buf hb_src, hb_aff, hb_sc, hb_out, hb_stats;
    grow_buf short_word, short_out;          // short scalars: [0] promise flag, [1] measured bit length; result held back until the flag is read
    grow_buf hb_idx, sel_flag, sel_gather;   // batch items: index lists, out-of-range flags, scalars gathered for one MSM
    size_t seg_chunk_terms = 0;              // amdmsm_set_segments_chunk_terms: terms a segmented MSM works through at a time, 0 = automatic
    void *seg_host = nullptr;                // segmented MSM: pinned staging of the slice descriptors (grow-only) and the
    size_t seg_host_bytes = 0;               // event behind their last upload, which the next call waits for before it
    hipEvent_t seg_copied = nullptr;         // overwrites them
    hipStream_t copy_stream = nullptr;
    hipEvent_t bases_ready = nullptr, host_done = nullptr;
    // Several MSMs in flight (pipeline depth > 1), overlap by construction: the bulk of every MSM -- bucket sort
    // and accumulation, which fill the device -- is enqueued on ONE stream in call order, its latency-bound tail
    // (bucket fix-up, reduction, Horner: a few waves, 0.6 ms of dependent chains at 2^20 points) on a second,
    // high-priority stream.  MSM k+1's sort and accumulation therefore start when MSM k's accumulation ends and
    // run under MSM k's tail; the accumulation kernel is launched one workgroup per CU short of full occupancy
    // in this mode so that a tail wave finds registers on every SIMD (group_vtable::accumulate_overlap).
    hipStream_t bulk_stream = nullptr, tail_stream = nullptr;
    std::vector<base_entry> bases;
    uint64_t next_base_id = 1, use_clock = 0;
    fb_state fb;
    stream_state ss;
    hipEvent_t aux_ev[5] = {};                    // phases of the last amdmsm_batch_exp
    // phase marks of the last timed call between call_begin and call_end (the group FFT, every Fr entry): the time from a
    // mark to the next belongs to the mark's phase, so the phases of all stages and chunks add up (grow-only; the ring
    // above holds one set of six events per call)
    std::vector<hipEvent_t> call_ev;
    std::vector<unsigned char> call_phase;
    size_t call_marks = 0;
    long long call_ticket = -1;
    float aux_ms[4] = {};
    // the last batch_exp was amdmsm_batch_exp_device, which does not wait: its times are read off aux_ev when asked for
    bool aux_pending = false, aux_reused = false, aux_normalised = false;
    fr_tw_entry fr_tw[4];                         // a prover alternates omega and omega^-1; a step domain has two transforms each way
    uint64_t fr_clock = 0;
    std::vector<fr_matrix *> fr_mats;
    std::string err;
    std::recursive_mutex mu;                      // one call at a time per context (entries nest)
};

namespace {

// The group translation units are linked weakly so a development build may carry a
// subset (AMDMSM_GROUPS=... python -m libff_amd.build); absent groups report UNSUPPORTED.
using vt_getter = const group_vtable *(*)();
const group_vtable *find_vt(int curve, int group) {
    static const vt_getter getters[] = {
        vt_alt_bn128_g1, vt_alt_bn128_g2, vt_bls12_377_g1, vt_bls12_377_g2, vt_bw6_761_g1, vt_bw6_761_g2,
        vt_bls12_381_g1, vt_bls12_381_g2, vt_mnt4_g1, vt_mnt4_g2, vt_mnt6_g1,
    };
    for (vt_getter g : getters) {
        if (!g) continue;
        const group_vtable *v = g();
        if (v->curve == curve && v->group == group) return v;
    }
    return nullptr;
}

// alignment of a libff record stride: the device loads coordinates 16 bytes at a time, 8 for the 10-word fields
size_t rec_align(const group_vtable *vt) { return vt->fq_words % 4 ? 8 : 16; }

thread_local std::string g_err_no_ctx;   // the last refusal of a call that was given no context
int fail(amdmsm_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    else g_err_no_ctx = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            return fail(ctx, AMDMSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                    \
    } while (0)

// libff::log2 (ceil), utils.cpp:32-44
size_t libff_log2(size_t n) {
    size_t r = ((n & (n - 1)) == 0 ? 0 : 1);
    while (n > 1) {
        n >>= 1;
        r++;
    }
    return r;
}

// One region of the MSM workspace: `unit` bytes for each of its units, from byte `off` on.  make_plan places the regions
// (place) and is the only place that writes a unit; every user takes the pointer of unit i from ws_at.
struct ws_region { size_t off = 0, unit = 0; };
template <class T = uint32_t>
T *ws_at(char *ws, const ws_region &r, size_t i = 0) {
    return (T *)(ws + r.off + i * r.unit);
}
struct plan_t {
    int c = 0, W = 0;
    int D = 0;   // > 0: precomputed-table mode, D digits per scalar in one bucket set (W == 1)
    int G = 1;   // window groups (see ws_slot)
    uint32_t B = 0, L = 0;
    uint32_t S = 0, T = 0;   // entries per accumulation lane, lanes per window
    size_t total = 0;
    // unit = one window, of the K * W the workspace holds: window ends and lists, bucket accumulators, the two levels of
    // the segment sums, first / last partial record and continued bucket of every lane, the sort's coarse counters,
    // cursors, payloads and fine keys
    ws_region counts, lists, buckets, lvl0, lvl1, pfirst, plast, cont, coarse, cursor, tmp_payload, tmp_key;
    ws_region rc, planes, winsum;   // the same for vt->reduce_rowcol (rowcol): row / column sums, bit planes, window sum
    ws_region big, endo;            // unit = one MSM of a batch: big-bin sort scratch; phi(P) = (beta x, y) of every base, compact affine
    ws_region queue;                // unit = one window group: its fix-up queue
    ws_region partial;              // unit = one Jacobian point: what the Horner chain of a window group hands to the next
    // bucket reduction as row / column sums + bit planes (vt->reduce_rowcol): serial lengths
    bool rowcol = false;
    uint32_t q_row = 0, q_col = 0;
    int K = 1;               // MSMs the workspace holds side by side (amdmsm_msm_device_batch)
    size_t list_stride = 0;  // words between two windows of `lists` (and of the sort's payloads and keys)
    bool glv = false;        // endomorphism split: the sorted columns are 2 * n_real half-length scalars
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// puts `count` units of `unit` bytes at *off and moves *off behind them, to the next multiple of 256
void place(ws_region &r, size_t *off, size_t count, size_t unit) {
    r.off = *off;
    r.unit = unit;
    *off = align_up(*off + count * unit, 256);
}
// the buffers of the sort of MSM j of the workspace (a single MSM: j = 0) -- its windows start at window j * W
sort_bufs sort_bufs_of(const plan_t &p, char *ws, size_t j) {
    const size_t w = j * (size_t)p.W;
    uint32_t *lists = ws_at(ws, p.lists, w);
    // the digits live in the lists' space
    return sort_bufs{ws_at(ws, p.coarse, w), ws_at(ws, p.cursor, w), (int32_t *)lists, ws_at(ws, p.tmp_payload, w),
                     ws_at(ws, p.tmp_key, w), ws_at(ws, p.counts, w), lists, p.list_stride, ws_at(ws, p.big, j)};
}

// Windows needed for signed radix-2^c digits of the half scalars of the endomorphism split,
// |k| <= 2^lb: the recoded top digit must not carry out, i.e. 2^lb < 2^(cW-1) - 2^(c(W-1))
// (the "+ 2" of field_get_signed_digit's bits + 2, multiexp.tcc:584-586, with the real bound in
// place of the bit length: alt_bn128 |k| < 2^125.8 fits 8 windows of 16 bits).
int glv_windows(const group_vtable *vt, int c) {
    const double lb = vt->glv_bound_log2_x1000 / 1000.0 + 1e-3;
    int W = 1;
    while ((double)(c * W - 1) + std::log2(1.0 - std::ldexp(1.0, 1 - c)) < lb) ++W;
    return W;
}
// sbits > 0: every scalar is known to be below 2^sbits (amdmsm_*_short), so the windows cover sbits + 2 bits -- what
// libff does with num_bits = max_i bi_exponents[i].num_bits() (multiexp.tcc:577-586)
int num_windows(const group_vtable *vt, int c, bool glv, int sbits = 0) {
    return glv ? glv_windows(vt, c) : ((sbits > 0 ? sbits : vt->fr_bits) + 2 + c - 1) / c;
}

// Window size.  Cost model fitted to measurements on MI355X (alt_bn128 G1, tools/sweep_c.py; the other
// fields scale every term alike, the wide ones pay more per bucket because their reduction
// kernels spill).  From 2^23 points up: sort + accumulation ~0.10 ns per (point, window) entry;
// fix-up + bucket reduction ~0.35 ms + 0.5 ns per bucket (0.98 ms for 16 x 2^16 buckets, 3.1 - 5.0
// for 13 x 2^19).  Below that the reduction is a latency floor (~0.65 ms from 2^16 points up) and
// c = 16 -- 2^15 buckets, exactly one reduction lane per SIMD lane -- is the measured optimum for
// every group from 2^16 to 2^22 points (c = 15 is slower even in the reduction: 0.74 vs 0.64 ms);
// the round-1 constants reproduce that and are kept there.  A top window that keeps only 2..8 significant bits concentrates all of
// its n entries in a handful of buckets, which the second sort level (one workgroup per coarse
// bin) processes almost serially -- such c are penalised rather than forbidden.
//
// (Round 3 re-sweep after the bucket reduction became plain sums, profiles/r03_sweep_c.txt: the choices below still hold --
// 2^16..2^21 c = 16 with the split (c = 13: 1.04 vs 0.68 ms at 2^16), 2^23 c = 17, 2^24..2^26 c = 20; bls12_377 G1 2^22 c = 17,
// bw6_761 G1 2^21 c = 16 (c = 14: 47.4 vs 45.2 ms), 2^24 c = 19; bls12_377 G2 2^21 c = 16 / 17, 2^24 c = 20.  A refit with
// per-field entry and bucket prices chose worse for the wide fields and was dropped.  Left on the table: alt_bn128 G1 2^22 with
// the split at c = 19 (7 windows) 7.16 vs 7.31-7.54 ms.)
// Modelled time (ns, alt_bn128 G1 scale) of an MSM over n points with window size c, with or without
// the endomorphism split.  The split doubles the digit columns and halves their length: about the
// same number of bucket entries, half the buckets to reduce and half the final doublings
// (~1.95 us each) -- measured on alt_bn128 G1 2^16 / 2^18 / 2^20 / 2^21 points: 1.02 vs 1.34,
// 1.34 vs 1.71, 2.66 vs 2.98, 4.38 vs 4.56 ms; its entries cost the same below 2^22 points and ~8 %
// more above, where bases plus phi(P) records (2 x 64 B x n) no longer fit the 256 MB Infinity
// Cache, so from 2^22 points up the plain path is level or ahead again (2^22: 7.78 vs 7.84,
// 2^23: 14.0 vs 13.7, 2^26: 87.4 vs 87.6 ms; profiles/r02_endomorphism_sweep.txt).
double plan_cost(const group_vtable *vt, size_t n, int c, bool glv, int sbits = 0) {
    const int bits = glv ? (vt->glv_bound_log2_x1000 + 999) / 1000 : (sbits > 0 ? sbits : vt->fr_bits);
    const int W = num_windows(vt, c, glv, sbits);
    const double cols = glv ? 2.0 * (double)n : (double)n;   // digit columns
    const double B = (double)((size_t)1 << (c - 1));
    // (24 limbs: the reduction kernels run one wave per SIMD; ~10 ns per bucket against 0.8 for 8 limbs,
    // while an accumulation entry costs 8.3x)
    const double wide = vt->fq_words >= 24 ? 2.2 : ((vt->fq_words > 8 || vt->el_words > vt->fq_words) ? 1.5 : 1.0);
    // (the wider fields hide the second base load behind their longer additions: same rate either way)
    // (round 3: with the cheaper reduction the split still wins a little above 2^22 points for the 8-limb field -- 2^22:
    // c = 19, 7 windows 7.16 ms against 7.3-7.5 plain; 2^23: 13.5 against 13.1 -- so its entries are priced level up to 5 M points;
    // with the reduced-radix accumulation: 2^23 12.0 either way, 2^24 21.8 (split, c = 19) against 22.8, 2^25 41.6 against 40.4,
    // 2^26 77.9 (c = 22) against 75.3 -- level up to 20 M points)
    const double entry = !glv ? 1.0 : (n < ((size_t)1 << 22) ? 1.0 : (wide > 1.0 ? 1.02 : (n < ((size_t)20 << 20) ? 1.0 : 1.08)));
    const bool large = n >= ((size_t)1 << 23);
    // windows that can hold a nonzero digit: with W * c well above the scalar length the top
    // window sees neither a scalar bit nor the carry (c = 17: 15 of 16 windows for a 254-bit
    // Fr) -- measured to pay from 2^23 points up (2^23: c = 17 14.4 ms vs c = 16 15.0 ms;
    // at 2^21 / 2^22 the accumulation time does not drop and c = 16 stays ahead)
    int W_work = W;
    if (large) {
        while (W_work > 1 && (W_work - 1) * c >= bits + 1) --W_work;
    }
    double cost;
    if (large) {
        cost = (double)W_work * cols * 0.10 * entry + 0.35e6 + (double)W * B * 0.5 * wide;
    } else {
        double reduce_cost = (double)W * B * 0.8 * wide;
        if (n >= 65536) reduce_cost = std::max(reduce_cost, 0.65e6);
        cost = (double)W * cols * 0.137 * entry + reduce_cost;
    }
    cost += (double)W * c * 1.95e3;   // final doublings
    const int top_bits = bits + 1 - (W - 1) * c;   // bit positions left for the top window
    if (top_bits >= 2 && top_bits <= 8) cost += cols * 3.0 / (double)(1 << (top_bits - 1));
    return cost;
}

// n: points
int choose_c(const group_vtable *vt, size_t n, bool glv = false, double *cost_out = nullptr, int sbits = 0) {
    if (n == 0) return 2;
    if (sbits > 0) {
        // short scalars: the measured table below was fitted to full-length scalars and does not apply; the model
        // alone decides, and a window wider than sbits + 2 bits would only add empty buckets
        double best = 1e300;
        int best_c = 2;
        for (int c = 2; c <= 22 && c <= sbits + 2; ++c) {
            const double cost = plan_cost(vt, n, c, false, sbits);
            if (cost < best) {
                best = cost;
                best_c = c;
            }
        }
        if (cost_out) *cost_out = best;
        return best_c;
    }
    // Small and medium inputs are launch and chain latency, which the model does not describe; the choice there is measured
    // (profiles/r04_experiments.txt, every group, c = 2 .. 16 at 2^2 .. 2^17 points).  Since the bucket reduction became plain sums
    // (row / column sums, bit planes: c >= 10) the short Horner of few wide windows wins over few buckets: c = 10 up to 2^10
    // points (alt_bn128 G2 n = 4: 1.41 ms against 3.19 at the c = 2 the model used to pick, bw6_761 G1 2.1 against 3.4),
    // c = 13 -- a square 64 x 64 weight matrix -- from there to where c = 16 takes over: 2^15 points for the prime-field groups
    // under the endomorphism split, 2^17 for Fq2 and 761-bit coordinates, 2^18 without the split (alt_bn128 G1 2^12: 0.49 ms
    // against 0.61 at c = 8; alt_bn128 G2 2^16: 1.93 against 2.36 at c = 16).  Round 2's rule (c = 8 below 2^16) dated from
    // the segment kernels.
    {
        const bool slow_field = vt->fq_words >= 24 || vt->el_words > vt->fq_words;
        const size_t n13 = !glv ? ((size_t)1 << 18) : (slow_field ? ((size_t)1 << 17) : ((size_t)1 << 15));
        int small_c = 0;
        if (n < 1024) small_c = 10;
        else if (n < n13) small_c = (vt->fq_words >= 24 && n < ((size_t)1 << 15)) ? 12 : 13;
        else if (n < 65536) small_c = 16;   // 2^15 points under the split: 0.54 ms against 0.57 at c = 13 and 0.70 at c = 8
        if (small_c) {
            if (cost_out) *cost_out = plan_cost(vt, n, small_c, glv);
            return small_c;
        }
    }
    double best = 1e300;
    int best_c = 2;
    for (int c = 2; c <= 22; ++c) {
        const double cost = plan_cost(vt, n, c, glv);
        if (cost < best) {
            best = cost;
            best_c = c;
        }
    }
    if (cost_out) *cost_out = best;
    return best_c;
}

// table_digits > 0: every scalar contributes table_digits entries (one per digit, pointing at
// its precomputed multiple) to a single bucket set; n is then the number of ENTRIES.
// glv: n counts the 2 x points digit columns of the endomorphism split
// batch > 1: workspace for `batch` MSMs side by side, each of at most n entries -- every per-window array holds batch * W windows, MSM j
// owning windows [j * W, (j + 1) * W), so that the tail kernels run once over all of them (amdmsm_msm_device_batch)
// What a caller asks of make_plan; a field left at its default is chosen by make_plan (c, L, S) or not in use.
struct plan_req {
    size_t entries = 0;          // n above: entries of one sorted list
    int c = 0, L = 0, S = 0;     // window bits, buckets per reduction lane, entries per accumulation lane
    int table_digits = 0;
    int groups = 0;              // window groups (see ws_slot)
    bool glv = false, overlap = false;
    int batch = 1;
    size_t big_words_min = 0;    // a batch of MSMs of different lengths: the largest big-bin scratch any of its lengths needs
    int sbits = 0;               // > 0: every scalar is below 2^sbits (see num_windows)
};
int make_plan(const group_vtable *vt, const plan_req &r, plan_t &p) {
    const size_t n = r.entries, big_words_min = r.big_words_min;
    const int c_req = r.c, L_req = r.L, S_req = r.S, table_digits = r.table_digits, G_req = r.groups, batch = r.batch, sbits = r.sbits;
    const bool glv = r.glv, overlap = r.overlap;
    if (c_req < 0 || c_req > 24 || c_req == 1) return AMDMSM_ERR_BAD_ARG;
    if (table_digits && (c_req < 2 || c_req > 22)) return AMDMSM_ERR_BAD_ARG;
    if (glv && (table_digits || c_req > 22)) return AMDMSM_ERR_BAD_ARG;
    p.glv = glv;
    p.c = c_req ? c_req : choose_c(vt, glv ? n / 2 : n, glv, nullptr, sbits);
    // field_get_signed_digit needs room for bits + 2 (multiexp.tcc:584-586)
    p.W = table_digits ? 1 : num_windows(vt, p.c, glv, sbits);
    p.D = table_digits;
    p.B = (uint32_t)1 << (p.c - 1);
    // buckets per reduction lane.  k_reduce_segments is bound by the dependent chain of one wave
    // (2 L additions + the segment-offset multiple + the 64:1 fold), so the best L is the one that
    // gives every SIMD about one wave: W * B / L ~ 65536 lanes (1024 waves), L in 2 .. 64.
    // Measured (alt_bn128 G1, reduction phase incl. fix-up): 2^20, c = 16: L = 4 / 8 / 16 ->
    // 0.86 / 0.66 / 0.84 ms; 2^23, c = 17: 8 / 16 / 32 -> 1.15 / 1.01 / 1.32; 2^26, c = 20:
    // 8 / 16 / 32 / 64 / 128 -> 6.80 / 5.43 / 5.09 / 5.09 / 5.62.
    // (groups whose reduction lanes are two physical lanes wide -- fp2h.cuh, reduce_fold == 32 --
    // need twice the L for the same wave count: bls12_377 G2 2^21 3.87 -> 2.96 ms with L = 16)
    const size_t red_lanes = (size_t)(64 / vt->reduce_fold);
    // The smallest L whose lanes the device holds at one wave per SIMD (65536, a few per cent more
    // still pays: bls12_381 G1, 17 windows of 2^15 buckets, L = 8 / 16 -> 69632 / 34816 lanes, 1.24 /
    // 1.53 ms), at most 64.  Window counts that are not powers of two used to land between one and
    // two waves per SIMD: bls12_377 G1 2^22 (15 x 2^16 buckets) L = 8 -> 16: 2.08 -> 1.83 ms,
    // bls12_377 G2 2^22 L = 16 -> 32: 5.36 -> 4.42 ms; bw6_761 G1 under the endomorphism split
    // (12 x 2^15) L = 4 / 8 / 16: 8.1 / 5.6 / 6.8 ms.
    uint32_t L = 2u;
    while (L < 64u && (size_t)p.W * (size_t)batch * p.B * red_lanes / L > (size_t)70000) L <<= 1;
    if (L_req > 0) L = (uint32_t)L_req;
    while (L > p.B) L >>= 1;
    if (L == 0 || (L & (L - 1))) return AMDMSM_ERR_BAD_ARG;
    p.L = L;
    const size_t xyz_bytes = (size_t)3 * vt->el_words * 4;
    p.list_stride = align_up(n ? n : 1, 64) + 16;   // + one chunk: a lane's last staged read may run past its entries
    // entries per lane S (<= 128, 256 in long launches; lane t of a window owns entries [t*S, (t+1)*S)).  All lanes do the
    // same work and the device holds `resident` of them at once, so the lane count W*T should
    // fill whole rounds: k rounds exactly for the smallest k that keeps S <= 128, or simply
    // S = 128 once there are many rounds anyway.
    {
        const double resident = (double)vt->accumulate_resident_lanes(overlap ? 1 : 0);
        const double entries = (double)n * p.W;
        uint32_t S = 8;
        if (entries >= 4.0 * 256.0 * resident) {
            // many rounds: longer lanes halve the partial records the fix-up and the export pass handle
            // (alt_bn128 G1, AMDMSM_ACC_S = 128 / 192 / 256 / 384 / 512: 2^26 75.5 / 74.8 / 74.0 / 74.1 / 74.6 ms,
            //  2^24 22.7 / 22.9 / 22.3 / 23.0 / 23.2 ms)
            S = 256;
        } else if (entries >= 8.0 * 128.0 * resident) {
            S = 128;
        } else if (entries > 8.0 * resident) {
            uint32_t k = 1;
            while (entries / (k * resident) > 128.0) ++k;
            S = (uint32_t)std::ceil(entries / (k * resident));
            while (S < 128 && (double)p.W * (double)((n + S - 1) / S) > k * resident) ++S;
        }
        if (S_req > 0) S = (uint32_t)S_req;
        p.S = S;
        p.T = (uint32_t)((n + S - 1) / S);
        if (p.T == 0) p.T = 1;
    }
    p.K = batch;
    const size_t Wt = (size_t)p.W * (size_t)batch;   // windows the workspace holds
    // The regions of the workspace, in the order they lie in it; the byte counts here are the only statement of a stride.
    size_t off = 0;
    place(p.counts, &off, Wt, p.B * 4);
    place(p.lists, &off, Wt, p.list_stride * 4);
    const size_t zz_bytes = (size_t)vt->bucket_words * 4;   // (X, Y, ZZ, ZZZ) bucket accumulators (reduced-radix groups: 4 L limbs)
    place(p.buckets, &off, Wt, p.B * zz_bytes);
    const size_t M = p.B / p.L;
    place(p.lvl0, &off, Wt, M * xyz_bytes);
    place(p.lvl1, &off, Wt, (M / 2 + 1) * xyz_bytes);   // first fold leaves at most M / 32 points
    place(p.pfirst, &off, Wt, p.T * zz_bytes);
    place(p.plast, &off, Wt, p.T * zz_bytes);
    place(p.cont, &off, Wt, p.T * 4);
    p.G = G_req > 0 ? std::min(std::min(G_req, MAX_GROUPS), p.W) : 1;
    // one fix-up queue per group, each sized for the largest group
    place(p.queue, &off, p.G, align_up(fixup_queue_words((size_t)((p.W + p.G - 1) / p.G) * (size_t)batch * p.T) * 4, 256));
    place(p.partial, &off, MAX_GROUPS, xyz_bytes);
    // two-level sort scratch.  The coarse counters, the cursors of the coarse pass and the header of the big-bin scratch
    // are cleared by ONE memset from coarse.off on, so these three regions must stay adjacent and in this order.
    place(p.coarse, &off, Wt, SORT_COARSE_WORDS * 4);
    place(p.cursor, &off, Wt, SORT_CURSOR_WORDS * 4);
    // (big_words_min: a batch of MSMs of different lengths passes the largest need of any of its lengths)
    place(p.big, &off, batch, p.c <= 22 ? align_up(std::max(sort_geometry(n, p.c, p.W).big_words, big_words_min) * 4, 256) : 256);
    place(p.tmp_payload, &off, Wt, p.list_stride * 4);
    place(p.tmp_key, &off, Wt, p.list_stride * 4);   // 16-bit fine keys use half of it
    place(p.endo, &off, batch, glv ? align_up((n / 2) * (size_t)vt->el_words * 2 * 4, 256) : 0);
    // Bucket reduction as plain sums (row / column sums of the weight matrix, bit planes, one short
    // Horner per window) from c = 10 up; below that a window's few segments fold inside one wave of
    // k_reduce_segments.  AMDMSM_ROWCOL=0 keeps the segment kernels everywhere (A/B runs).
    // Lanes add q buckets serially before the butterfly: the smallest q (>= 4 / 4) that keeps the
    // row and column lanes together within about two waves per SIMD -- measured: see make_plan's note
    // in profiles/r03_experiments.txt.
    {
        static const int rc_env = getenv("AMDMSM_ROWCOL") ? atoi(getenv("AMDMSM_ROWCOL")) : 1;
        static const int rc_min_c = getenv("AMDMSM_ROWCOL_MIN_C") ? atoi(getenv("AMDMSM_ROWCOL_MIN_C")) : 10;
        static const int qr_env = getenv("AMDMSM_ROWCOL_QROW") ? atoi(getenv("AMDMSM_ROWCOL_QROW")) : 0;
        static const int qc_env = getenv("AMDMSM_ROWCOL_QCOL") ? atoi(getenv("AMDMSM_ROWCOL_QCOL")) : 0;
        p.rowcol = rc_env != 0 && p.c >= rc_min_c;
        const int h = p.c / 2;
        const size_t C = (size_t)1 << h, R = p.B >> h;
        // (measured, tools/exp_rowcol.sh: alt_bn128 G1 2^20 q = 4 / 8 / 16 -> reduction phase 0.46 / 0.51 / 0.51 ms, 2^23
        // 1.09 / 0.87 / 0.79; the wide fields, whose kernels hold one wave per SIMD, want one round of lanes:
        // bw6_761 G1 2^21 q = 8 / 16 / 32 -> 5.41 / 5.03 / 6.24 ms, bls12_377 G2 2^21 2.72 / 2.57 / 3.07)
        const bool one_wave = vt->fq_words >= 24 || vt->el_words > vt->fq_words;
        const size_t lane_budget = one_wave ? 70000 : 140000;
        uint32_t q = 4;
        while (q < 64 && Wt * p.B * red_lanes * 2 / q > lane_budget) q <<= 1;
        p.q_row = qr_env > 0 ? (uint32_t)qr_env : q;
        p.q_col = qc_env > 0 ? (uint32_t)qc_env : q;
        place(p.rc, &off, Wt, (R + 1 + C) * xyz_bytes);
        place(p.planes, &off, Wt, p.c * xyz_bytes);
        place(p.winsum, &off, Wt, xyz_bytes);
    }
    p.total = off;
    return AMDMSM_OK;
}

int ensure_ws(amdmsm_ctx *ctx, ws_slot &sl, size_t bytes) {
    if (sl.ws_bytes >= bytes) return AMDMSM_OK;
    if (sl.ws) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipFree(sl.ws));
        sl.ws = nullptr;
        sl.ws_bytes = 0;
    }
    const size_t want = bytes + bytes / 8;
    HIP_TRY(ctx, hipMalloc(&sl.ws, want));
    sl.ws_bytes = want;
    return AMDMSM_OK;
}

constexpr uint64_t TIMING_RING = 64;
// The events of `ring`, aux_ev and call_ev only measure time, so they are created with hipEventDisableSystemFence: a
// plain event writes the caches back and invalidates them where it is recorded -- six times inside every timed call --
// and the kernels behind it pay for that (2^20 points: 1.593 -> 1.578 ms per step, profiles/digit_pass_and_step_gaps.txt).
// The flag is right for them because their only readers are hipEventElapsedTime calls behind an event or stream
// synchronisation of the reader's own, and nothing on the host looks at memory on the strength of one of them.
// ctx->ev keeps the default flags: amdmsm_mul_bench_device / amdmsm_madd_bench_device return behind a synchronisation on
// the event itself, and their callers then read what the probe kernel wrote.  The events that order streams (done,
// tail_done, acc_done, ov_*, bases_ready, host_done) keep theirs too.  AMDMSM_TIMING_NOFENCE=0: plain events (A/B runs).
hipError_t timing_event(hipEvent_t *e) {
    static const bool nofence = !(getenv("AMDMSM_TIMING_NOFENCE") && atoi(getenv("AMDMSM_TIMING_NOFENCE")) == 0);
    return nofence ? hipEventCreateWithFlags(e, hipEventDisableSystemFence) : hipEventCreate(e);
}
void record(amdmsm_ctx *ctx, ws_slot &, int idx, hipStream_t st) {
    if (ctx->timing) (void)hipEventRecord(ctx->ring[ctx->ticket % TIMING_RING][idx], st);
}

// The whole single-GPU MSM on device-resident inputs.
// table_digits > 0: d_bases is a precompute_table with that many multiples per scalar
// (multi_exp_precompute_from_fifo, multiexp_stream.tcc:124-162: one bucket set, no doublings).
// before_accumulate (optional): called once the bucket sort has been enqueued -- the sort reads
// only the scalars, so a host entry uses it to bring the bases in on another stream meanwhile;
// it returns an event the accumulation must wait for (or null).
// The endomorphism split (msm_group.hip glv_split) computes k P as k1 P + k2 phi(P), which equals
// k P exactly where phi = [lambda]: on the order-r subgroup.  opts->endomorphism: 0 = permitted only
// for groups whose whole curve has order r (alt_bn128 G1: every base qualifies), 1 = permitted: the
// caller guarantees subgroup membership of every base (libff's G1 / G2 are that subgroup; the FFI
// entry points check it while decoding), 2 = the same guarantee, and use it whatever the size,
// -1 = never.  Where permitted it is used when the cost model favours it (plan_cost).
// AMDMSM_GLV=off switches it off everywhere; AMDMSM_GLV=on|force apply only where the caller left
// the option at 0 (experiments; logged once) -- a caller's -1 is never overridden.
int glv_env() {
    static const int env = [] {
        const char *e = getenv("AMDMSM_GLV");
        int v = 0;
        if (!e) return 0;
        if (!strcmp(e, "off") || !strcmp(e, "0")) v = -1;
        else if (!strcmp(e, "on") || !strcmp(e, "1")) v = 1;
        else if (!strcmp(e, "all") || !strcmp(e, "force") || !strcmp(e, "2")) v = 2;
        else if (!strcmp(e, "auto")) v = 3;
        if (v) fprintf(stderr, "[amdmsm] AMDMSM_GLV=%s overrides amdmsm_opts.endomorphism where the caller left it at 0 "
                               "(off: everywhere); on / force assert that every base lies in the order-r subgroup\n", e);
        return v;
    }();
    return env;
}
// The permission half of the rule, without a cost model: 0 = the split may not be used, 1 = permitted, 2 = permitted
// and asked for at every size.
int endomorphism_permitted(const group_vtable *vt, const amdmsm_opts *opts) {
    const int env = glv_env();
    if (!vt->has_endomorphism) return 0;   // MNT4 / MNT6: every amdmsm_opts.endomorphism value is ignored
    int want = opts ? opts->endomorphism : 0;
    // The environment may switch the split off everywhere, and otherwise speaks only where the caller
    // expressed no choice (0): a caller's -1 (never) stays never, a caller's 1 / 2 keeps its meaning.
    if (env == -1) want = -1;
    else if ((env == 1 || env == 2) && want == 0) want = env;
    if (want < 0 || (want == 0 && !vt->prime_order)) return 0;
    return want >= 2 ? 2 : 1;
}
bool use_endomorphism(const group_vtable *vt, size_t n, const amdmsm_opts *opts, int table_digits) {
    const int permitted = endomorphism_permitted(vt, opts);
    if (!permitted) return false;
    if (table_digits || n == 0 || n >= ((size_t)1 << 30)) return false;
    const int c_req = opts ? opts->window_bits : 0;
    if (c_req > 22) return false;
    if (permitted >= 2) return true;
    // permitted: used where the model says it pays (small and medium inputs)
    double full = 0, split = 0;
    if (c_req) {
        full = plan_cost(vt, n, c_req, false);
        split = plan_cost(vt, n, c_req, true);
    } else {
        choose_c(vt, n, false, &full);
        choose_c(vt, n, true, &split);
    }
    return split < 0.98 * full;
}

int check_opts(amdmsm_ctx *ctx, const amdmsm_opts *opts) {
    if (opts && opts->struct_size != sizeof(amdmsm_opts))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "amdmsm_opts.struct_size does not match this library (AMDMSM_ABI_VERSION " +
                                                 std::to_string(AMDMSM_ABI_VERSION) + "): initialise with AMDMSM_OPTS_INIT");
    return AMDMSM_OK;
}
#define CHECK_OPTS(ctx, opts)                       \
    do {                                            \
        const int rc_opts_ = check_opts(ctx, opts); \
        if (rc_opts_) return rc_opts_;              \
    } while (0)

// the stream a device entry launches on
hipStream_t stream_of(const amdmsm_ctx *ctx, const amdmsm_opts *opts) {
    return (opts && opts->stream) ? (hipStream_t)opts->stream : ctx->stream;
}
// the caller's options, or the defaults of an entry called without any
amdmsm_opts opts_or_default(const amdmsm_opts *opts) {
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    if (opts) o = *opts;
    else o.out_form = AMDMSM_OUT_LIBFF;
    return o;
}

// One MSM handles at most this many points (its sorted lists index points with 31 bits, and the
// workspace grows with n: 42 GiB at 2^28 alt_bn128 points); longer inputs are cut into contiguous
// ranges whose partial results are summed, exactly the reference's chunk loop (multiexp.tcc:655-687).
// AMDMSM_MAX_RANGE_POINTS lowers the limit so that tests reach the split with small inputs.
constexpr size_t MAX_RANGES = 64;
size_t max_range_points() {
    static const size_t v = [] {
        const char *e = getenv("AMDMSM_MAX_RANGE_POINTS");
        const long long x = e ? atoll(e) : 0;
        return x > 0 ? (size_t)x : (size_t)1 << 28;
    }();
    return v;
}

struct msm_hook {
    int (*fn)(void *arg, hipEvent_t *wait_for) = nullptr;
    void *arg = nullptr;
};
// Scalars known to be short (amdmsm_*_short), once the entry point has settled how the call runs: the digit pass reads
// elements of `kind`, the plan's windows cover `bits` + 2 bits, no endomorphism split.
struct short_spec {
    int kind = 0;               // AMDMSM_SCALAR_*
    int bits = 0;               // 1 .. below Fr::num_bits
    uint32_t *flag = nullptr;   // device word the digit pass raises for a scalar >= 2^bits; null: nothing to test
    bool uploaded = false;      // host entry: the scalars are already in ctx->hb_sc (the measuring pass brought them)
    size_t elem_bytes(const group_vtable *vt) const { return kind ? (size_t)kind : (size_t)vt->fr_words * 4; }
};
// bits the digit pass tests against: the kind's full width where there is nothing to test
int short_limit_bits(const group_vtable *vt, const short_spec &ss) {
    return ss.flag ? ss.bits : (ss.kind ? 8 * ss.kind : 32 * vt->fr_words);
}
// The tail of an MSM in front of its Horner chain, for the nw windows [w0, w0 + nw) of the workspace ws, on stream ts:
// the fix-up of the buckets that span accumulation lanes (fix-up queue `queue`), then the bucket reduction -- row / column
// sums and bit planes, or segment sums and the levels that fold them.  Returns the nw window sums Horner reads.
uint32_t *enqueue_tail(const group_vtable *vt, const plan_t &p, char *ws, int w0, int nw, hipStream_t ts, int queue) {
    const size_t w = (size_t)w0;
    uint32_t *buckets = ws_at(ws, p.buckets, w);
    vt->accumulate_fixup(ts, ws_at(ws, p.counts, w), buckets, ws_at(ws, p.pfirst, w), ws_at(ws, p.plast, w), ws_at(ws, p.cont, w),
                         ws_at(ws, p.queue, (size_t)queue), nw, p.B, p.S, p.T);
    if (p.rowcol) {
        uint32_t *winsum = ws_at(ws, p.winsum, w);
        vt->reduce_rowcol(ts, buckets, nw, p.B, p.c, p.q_row, p.q_col, ws_at(ws, p.rc, w), ws_at(ws, p.planes, w), winsum);
        return winsum;
    }
    uint32_t *src = ws_at(ws, p.lvl0, w), *dst = ws_at(ws, p.lvl1, w);
    vt->reduce_segments(ts, buckets, nw, p.B, p.L, src);
    const uint32_t fold = (uint32_t)vt->reduce_fold;
    uint32_t M = p.B / p.L;   // segments of a window
    M /= std::min<uint32_t>(M, fold);   // folded per wave inside reduce_segments
    while (M > 1) {
        if ((size_t)M * (64 / fold) <= 256) {   // the remaining levels in one launch
            vt->sum_block(ts, src, nw, M, dst);
            M = 1;
        } else {
            vt->sum_butterfly(ts, src, nw, M, dst);
            M /= std::min<uint32_t>(M, fold);
        }
        std::swap(src, dst);
    }
    return src;
}

int msm_device_impl(amdmsm_ctx *ctx, const group_vtable *vt, const uint32_t *d_bases, const uint32_t *d_scalars,
                    size_t n, uint32_t *d_out, const amdmsm_opts *opts, int table_digits = 0,
                    const msm_hook *hook = nullptr, const uint32_t *d_endo_resident = nullptr, const short_spec *ss = nullptr) {
    hipStream_t st = stream_of(ctx, opts);
    hipStream_t const user_st = st;
    const int form = opts ? opts->out_form : AMDMSM_OUT_LIBFF;
    const int mont = (opts && opts->scalars_plain) ? 0 : 1;
    static const bool atomic_env = getenv("AMDMSM_SORT") && !strcmp(getenv("AMDMSM_SORT"), "atomic");
    const bool atomic_sort = atomic_env && !ss;   // the short digit pass exists for the two-level sort only
    const bool glv = !ss && use_endomorphism(vt, n, opts, table_digits) && !atomic_sort;
    const size_t entries = table_digits ? n * (size_t)table_digits : (glv ? 2 * n : n);   // per sorted list
    if (entries >= ((size_t)1 << 31)) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n (times table digits) must be < 2^31 per call");
    if (n == 0) {
        // empty sum = zero; sum_points over 0 points writes G::zero() in the requested form
        vt->sum_points(st, d_out, 0, form, d_out);
        HIP_TRY(ctx, hipGetLastError());
        return AMDMSM_OK;
    }
    plan_t p;
    // tuning knobs for experiments: AMDMSM_ACC_S (entries per accumulation lane)
    static const int acc_s_env = getenv("AMDMSM_ACC_S") ? atoi(getenv("AMDMSM_ACC_S")) : 0;
    static const int groups_env = getenv("AMDMSM_WINDOW_GROUPS") ? atoi(getenv("AMDMSM_WINDOW_GROUPS")) : 0;
    // overlap mode (several MSMs in flight, see amdmsm_ctx::bulk_stream): built and parity-tested, but OFF unless
    // AMDMSM_OVERLAP=1 -- measured on MI355X / ROCm 7.2 it loses (2^20, three in flight: 2.35 - 2.69 ms per MSM against
    // 2.09 - 2.14 with the ordering left to the hardware queues and 2.19 one at a time): the kernel traces in
    // profiles/r03_pipelined_*.txt show the intended schedule (sort and accumulation of MSM k+1 under the tail of MSM k)
    // but every kernel behind a cross-queue event wait starts ~50 us late, which outweighs the 0.7 ms tail it hides.
    static const bool overlap_env = getenv("AMDMSM_OVERLAP") && atoi(getenv("AMDMSM_OVERLAP")) != 0;
    const bool overlap = overlap_env && ctx->depth > 1 && ctx->bulk_stream && vt->accumulate_overlap_ok && !groups_env;
    plan_req req;
    req.entries = entries;
    req.c = opts ? opts->window_bits : 0;
    req.L = opts ? opts->segment_len : 0;
    req.S = acc_s_env;
    req.table_digits = table_digits;
    req.groups = groups_env;
    req.glv = glv;
    req.overlap = overlap;
    req.sbits = ss ? ss->bits : 0;
    int rc = make_plan(vt, req, p);
    if (rc) return fail(ctx, rc, "bad window_bits / segment_len");
    if (ss && p.c > 22) return fail(ctx, AMDMSM_ERR_BAD_ARG, "window_bits > 22 is not available for short scalars");
    const int slot_idx = (int)(ctx->next++ % (unsigned)ctx->depth);
    ws_slot &sl = ctx->slots[slot_idx];
    ctx->last_slot = slot_idx;
    if (overlap) {
        // the bulk part runs on the context's bulk stream, behind whatever the caller's stream holds now
        HIP_TRY(ctx, hipEventRecord(sl.ov_in, user_st));
        st = ctx->bulk_stream;
        HIP_TRY(ctx, hipStreamWaitEvent(st, sl.ov_in, 0));
    }
    if (sl.used) HIP_TRY(ctx, hipStreamWaitEvent(st, sl.done, 0));   // previous user of this slot
    rc = ensure_ws(ctx, sl, p.total);
    if (rc) return rc;
    char *ws = (char *)sl.ws;
    const sort_bufs sb = sort_bufs_of(p, ws, 0);

    record(ctx, sl, 0, st);
    // phi(P) of every base (endomorphism split): independent of the sort, so it runs beside it on
    // the slot's side stream when the bases are already on the device (no upload hook)
    // (d_endo_resident: the records already exist, kept with a registered base vector)
    const uint32_t *endo_pts = !glv ? nullptr : (d_endo_resident ? d_endo_resident : ws_at(ws, p.endo));
    const bool endo_beside = glv && !d_endo_resident && !(hook && hook->fn);
    // the side stream also clears the bucket array and the queue heads while the sort runs (both
    // are first touched by the accumulation)
    HIP_TRY(ctx, hipEventRecord(sl.tail_done[0], st));
    if ((atomic_sort || p.c > 22) && !table_digits) {
        HIP_TRY(ctx, hipMemsetAsync(sb.ends, 0, (size_t)p.W * p.counts.unit, st));
        vt->count(st, d_scalars, n, mont, p.c, p.W, sb.ends);
        record(ctx, sl, 1, st);
        vt->scatter(st, d_scalars, n, mont, p.c, p.W, sb.ends, sb.lists, p.list_stride);
    } else {
        HIP_TRY(ctx, hipMemsetAsync(sb.coarse, 0, p.big.off + 16 - p.coarse.off, st));   // counters + cursors + big-bin header
        record(ctx, sl, 1, st);
        if (ss)
            vt->sort(st, sort_src::short_scalars(d_scalars, ss->kind, short_limit_bits(vt, *ss), ss->flag), n, mont, p.c, p.W, sb, 0);
        else
            vt->sort(st, sort_src::own(d_scalars), n, mont, p.c, table_digits ? table_digits : p.W, sb,
                     table_digits ? 1 : (glv ? 2 : 0));
    }
    // (measured at 2^20 points: beside the whole sort 0.29 ms for the phase, beside its LDS-bound
    // second half only 0.35, after it 0.30; the plain path's sort takes 0.24)
    // enqueued after the sort kernels, ordered only behind the start of the call
    // (overlap mode keeps them on the bulk stream: the runtime multiplexes the many streams of a process over a few
    // hardware queues, and a side stream that lands in the queue of a caller's stream sits behind that stream's wait
    // for the previous MSM's tail -- seen in a kernel trace: the accumulation then started only after that tail)
    hipStream_t side = overlap ? st : sl.side[0];
    if (!overlap) HIP_TRY(ctx, hipStreamWaitEvent(side, sl.tail_done[0], 0));
    HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.buckets), 0, (size_t)p.W * p.buckets.unit, side));
    for (int g = 0; g < p.G; ++g) HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.queue, (size_t)g), 0, 8, side));
    if (endo_beside) vt->endo_points(side, d_bases, n, ws_at(ws, p.endo));
    if (!overlap) HIP_TRY(ctx, hipEventRecord(sl.acc_done[0], side));
    if (hook && hook->fn) {
        hipEvent_t wait_for = nullptr;
        rc = hook->fn(hook->arg, &wait_for);
        if (rc) return rc;
        if (wait_for) HIP_TRY(ctx, hipStreamWaitEvent(st, wait_for, 0));
    }
    if (!overlap) HIP_TRY(ctx, hipStreamWaitEvent(st, sl.acc_done[0], 0));
    if (glv && !d_endo_resident && !endo_beside) vt->endo_points(st, d_bases, n, ws_at(ws, p.endo));
    // groups of windows, highest first: [w0, w0 + wg)
    int w_hi = p.W;
    for (int g = 0; g < p.G; ++g) {
        const int wg = p.W / p.G + (g < p.W % p.G ? 1 : 0);
        const int w0 = w_hi - wg;
        w_hi = w0;
        const bool last = g == p.G - 1;
        // accumulation group after group on the caller's stream; the tail of a finished group
        // moves to a side stream
        hipStream_t ts = last ? (overlap ? ctx->tail_stream : st) : sl.side[g];
        if (g == 0) record(ctx, sl, 2, st);
        vt->accumulate(st, ws_at(ws, p.counts, w0), ws_at(ws, p.lists, w0), p.list_stride, d_bases, ws_at(ws, p.buckets, w0),
                       ws_at(ws, p.pfirst, w0), ws_at(ws, p.plast, w0), ws_at(ws, p.cont, w0), wg, p.B, p.S, p.T, endo_pts, n,
                       overlap ? 1 : 0);
        if (last) {
            record(ctx, sl, 3, st);
            if (overlap) {
                HIP_TRY(ctx, hipEventRecord(sl.ov_acc, st));
                HIP_TRY(ctx, hipStreamWaitEvent(ts, sl.ov_acc, 0));
            }
        } else {
            HIP_TRY(ctx, hipEventRecord(sl.acc_done[g], st));
            HIP_TRY(ctx, hipStreamWaitEvent(ts, sl.acc_done[g], 0));
        }
        const uint32_t *src = enqueue_tail(vt, p, ws, w0, wg, ts, g);
        // Horner over this group's windows, continuing from the groups above
        if (g > 0) HIP_TRY(ctx, hipStreamWaitEvent(ts, sl.tail_done[g - 1], 0));
        if (last) record(ctx, sl, 4, ts);
        vt->horner(ts, src, wg, p.c, last ? form : (int)AMDMSM_OUT_JACOBIAN, g > 0 ? ws_at(ws, p.partial, g - 1) : nullptr,
                   last ? d_out : ws_at(ws, p.partial, g));
        if (!last) HIP_TRY(ctx, hipEventRecord(sl.tail_done[g], ts));
    }
    if (overlap) {
        // the result (and the slot) belong to the caller's stream again once the tail has run
        record(ctx, sl, 5, ctx->tail_stream);
        HIP_TRY(ctx, hipEventRecord(sl.ov_tail, ctx->tail_stream));
        HIP_TRY(ctx, hipStreamWaitEvent(user_st, sl.ov_tail, 0));
        st = user_st;
    } else {
        record(ctx, sl, 5, st);
    }
    if (ctx->timing) sl.last_ticket = (long long)ctx->ticket++;
    sl.ev_valid = ctx->timing;
    HIP_TRY(ctx, hipEventRecord(sl.done, st));
    sl.used = true;
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

constexpr int MAX_BATCH = 8;   // MSMs of one batch call
int ensure_buf(amdmsm_ctx *ctx, grow_buf &b, size_t bytes);

// One MSM of a ragged batch, every pointer an HBM address (amdmsm_batch_item after upload / as the device entry got it).
struct item_dev {
    const uint32_t *bases = nullptr;
    size_t n = 0;
    const uint32_t *scalars = nullptr;   // own vector; null: shared[index[i]] or shared[offset + i]
    size_t offset = 0;
    const uint32_t *index = nullptr;
    uint32_t *out = nullptr;
};

// k MSMs of one group, each of its own length n_j, in one pass (the batch entries, equal-length and ragged).  Sort and
// accumulation fill the device and run MSM after MSM; the tail -- fix-up, bucket reduction, final Horner: dependent chains
// of a few waves, a quarter of a 2^20-point MSM -- runs ONCE over the k * W windows of all of them, so its latency is paid
// once per batch instead of once per MSM (2^20 points, k = 3: see profiles/r03_experiments.txt).  This is the overlap a
// prover's back-to-back MSMs can really have on this device: in one stream, by making the latency-bound kernels wider.
// ONE plan for the batch -- window size, window count, endomorphism decision and lane length are those of the longest
// MSM: sort and accumulation are linear in the entries, so the longest MSM carries most of their cost and is served
// best by its own optimum, while the shared tail depends on (k W, B, c) only.  (Minimising the summed plan_cost would
// also have to re-derive the measured small-size rules of choose_c for mixtures; with one long MSM beside short ones --
// the prover's shape -- both rules pick the same c.)  Every per-MSM stride of the workspace is sized for that longest
// MSM; a shorter one uses the front of its share, an empty one launches nothing and has its window ends and lane
// markers cleared so that the shared tail finds empty windows.
// flags: k words, zeroed here; word j becomes nonzero when MSM j named an element at or past shared_n.  Null where every
// MSM brings its own scalars (the equal-length entries): nothing is cleared and no MSM may select from d_shared.
int msm_device_batch_items_impl(amdmsm_ctx *ctx, const group_vtable *vt, int k, const item_dev *it, const uint32_t *d_shared,
                                size_t shared_n, uint32_t *flags, const amdmsm_opts *opts) {
    hipStream_t st = stream_of(ctx, opts);
    const int form = opts ? opts->out_form : AMDMSM_OUT_LIBFF;
    const int mont = (opts && opts->scalars_plain) ? 0 : 1;
    size_t n_max = 0;
    for (int j = 0; j < k; ++j) n_max = std::max(n_max, it[j].n);
    if (flags) HIP_TRY(ctx, hipMemsetAsync(flags, 0, (size_t)k * 4, st));
    if (n_max == 0) {
        for (int j = 0; j < k; ++j) vt->sum_points(st, it[j].out, 0, form, it[j].out);
        HIP_TRY(ctx, hipGetLastError());
        return AMDMSM_OK;
    }
    const bool glv = use_endomorphism(vt, n_max, opts, 0);
    const size_t entries = glv ? 2 * n_max : n_max;
    plan_req req;
    req.entries = entries;
    req.c = opts ? opts->window_bits : 0;
    req.L = opts ? opts->segment_len : 0;
    req.glv = glv;
    req.batch = k;
    plan_t p;
    int rc = make_plan(vt, req, p);
    if (rc) return fail(ctx, rc, "bad window_bits / segment_len");
    if (p.c > 22) return fail(ctx, AMDMSM_ERR_BAD_ARG, "window_bits > 22 is not available for a batch");
    // the sort geometry (coarse bits, chunk size, big-bin scratch) follows each MSM's own length: the scratch
    // of every MSM is sized for the largest need of any length in the batch, planned again with the c just chosen
    req.c = p.c;
    for (int j = 0; j < k; ++j) {
        if (it[j].n) req.big_words_min = std::max(req.big_words_min, sort_geometry(glv ? 2 * it[j].n : it[j].n, p.c, p.W).big_words);
    }
    rc = make_plan(vt, req, p);
    if (rc) return fail(ctx, rc, "bad window_bits / segment_len");
    const int slot_idx = (int)(ctx->next++ % (unsigned)ctx->depth);
    ws_slot &sl = ctx->slots[slot_idx];
    ctx->last_slot = slot_idx;
    if (sl.used) HIP_TRY(ctx, hipStreamWaitEvent(st, sl.done, 0));
    rc = ensure_ws(ctx, sl, p.total);
    if (rc) return rc;
    char *ws = (char *)sl.ws;
    const size_t Wt = (size_t)p.W * (size_t)k;
    record(ctx, sl, 0, st);
    HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.coarse), 0, p.big.off - p.coarse.off, st));   // counters + cursors
    for (int j = 0; j < k; ++j) HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.big, (size_t)j), 0, 16, st));
    HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.buckets), 0, Wt * p.buckets.unit, st));
    HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.queue), 0, 8, st));
    record(ctx, sl, 1, st);
    bool first = true;
    for (int j = 0; j < k; ++j) {
        const size_t w0 = (size_t)j * p.W, n = it[j].n;
        const sort_bufs sb = sort_bufs_of(p, ws, (size_t)j);
        if (n == 0) {
            // no entries: every bucket of its windows ends at 0 and no lane continues a bucket (NO_BUCKET = ~0)
            HIP_TRY(ctx, hipMemsetAsync(sb.ends, 0, (size_t)p.W * p.counts.unit, st));
            HIP_TRY(ctx, hipMemsetAsync(ws_at(ws, p.cont, w0), 0xff, (size_t)p.W * p.cont.unit, st));
            continue;
        }
        const sort_src src_j = it[j].scalars ? sort_src::own(it[j].scalars)
                                             : sort_src::selected(d_shared, shared_n, it[j].index, it[j].offset, flags + j);
        vt->sort(st, src_j, n, mont, p.c, p.W, sb, glv ? 2 : 0);
        uint32_t *endo_j = glv ? ws_at(ws, p.endo, (size_t)j) : nullptr;
        if (glv) vt->endo_points(st, it[j].bases, n, endo_j);
        if (first) record(ctx, sl, 2, st);
        first = false;
        vt->accumulate(st, sb.ends, sb.lists, p.list_stride, it[j].bases, ws_at(ws, p.buckets, w0), ws_at(ws, p.pfirst, w0),
                       ws_at(ws, p.plast, w0), ws_at(ws, p.cont, w0), p.W, p.B, p.S, p.T, endo_j, n, 0);
    }
    record(ctx, sl, 3, st);
    const uint32_t *src = enqueue_tail(vt, p, ws, 0, (int)Wt, st, 0);
    record(ctx, sl, 4, st);
    uint32_t *outs[MAX_BATCH];
    for (int j = 0; j < k; ++j) outs[j] = it[j].out;
    vt->horner_batch(st, src, k, p.W, p.c, form, outs);
    record(ctx, sl, 5, st);
    if (ctx->timing) sl.last_ticket = (long long)ctx->ticket++;
    sl.ev_valid = ctx->timing;
    HIP_TRY(ctx, hipEventRecord(sl.done, st));
    sl.used = true;
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int ensure_partials(amdmsm_ctx *ctx) {
    if (!ctx->chunk_partials) HIP_TRY(ctx, hipMalloc(&ctx->chunk_partials, MAX_RANGES * 3 * 24 * 2 * 4));
    return AMDMSM_OK;
}

// Device-resident MSM of any length: one msm_device_impl, or -- above max_range_points() -- the
// reference's chunk loop (multiexp.tcc:655-687: `one = total / chunks`, the last range takes the
// remainder, partial results summed) with ranges run one after the other on the caller's stream.
int msm_device_ranges(amdmsm_ctx *ctx, const group_vtable *vt, const uint32_t *d_bases, const uint32_t *d_scalars, size_t n,
                      uint32_t *d_out, const amdmsm_opts *opts, const short_spec *ss = nullptr) {
    const size_t maxr = max_range_points();
    if (n <= maxr) return msm_device_impl(ctx, vt, d_bases, d_scalars, n, d_out, opts, 0, nullptr, nullptr, ss);
    const size_t parts = (n + maxr - 1) / maxr;
    if (parts > MAX_RANGES) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "input too large for one call");
    const size_t one = (n + parts - 1) / parts;   // <= maxr: no range exceeds the limit, the last one takes what is left
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    const size_t fr_bytes = ss ? ss->elem_bytes(vt) : (size_t)vt->fr_words * 4;   // one bit length for all ranges
    int rc = ensure_partials(ctx);
    if (rc) return rc;
    amdmsm_opts o = opts_or_default(opts);
    const int form = o.out_form;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    hipStream_t st = stream_of(ctx, &o);
    for (size_t k = 0; k < parts; ++k) {
        const size_t lo = k * one, cnt = (k == parts - 1) ? n - lo : one;
        rc = msm_device_impl(ctx, vt, (const uint32_t *)((const char *)d_bases + lo * aff_bytes),
                             (const uint32_t *)((const char *)d_scalars + lo * fr_bytes), cnt,
                             (uint32_t *)((char *)ctx->chunk_partials + k * xyz_bytes), &o, 0, nullptr, nullptr, ss);
        if (rc) return rc;
    }
    vt->sum_points(st, (const uint32_t *)ctx->chunk_partials, (int)parts, form, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));   // the partials buffer is shared by the context
    return AMDMSM_OK;
}

// A ragged batch on device-resident inputs: one pass where its limits hold (k <= 8, sum n_j < 2^30, every n_j within one
// range), otherwise the MSMs one after the other through the single-MSM path, the scalars of an MSM that selects from
// the shared vector gathered on the device first (same selection, same guard).  flags (nullable): see msm_device_batch_items_impl.
int run_batch_items(amdmsm_ctx *ctx, const group_vtable *vt, int k, const item_dev *it, const uint32_t *d_shared, size_t shared_n,
                    uint32_t *flags, const amdmsm_opts *opts) {
    size_t sum = 0, n_max = 0;
    for (int j = 0; j < k; ++j) {
        sum += it[j].n;
        n_max = std::max(n_max, it[j].n);
    }
    if (n_max <= max_range_points() && sum < ((size_t)1 << 30))
        return msm_device_batch_items_impl(ctx, vt, k, it, d_shared, shared_n, flags, opts);
    if (opts && opts->window_bits > 22) return fail(ctx, AMDMSM_ERR_BAD_ARG, "window_bits > 22 is not available for a batch");
    hipStream_t st = stream_of(ctx, opts);
    const size_t fr_bytes = (size_t)vt->fr_words * 4;
    if (flags) HIP_TRY(ctx, hipMemsetAsync(flags, 0, (size_t)k * 4, st));
    for (int j = 0; j < k; ++j) {
        const uint32_t *sc = it[j].scalars;
        if (!sc && it[j].n) {
            const int rc = ensure_buf(ctx, ctx->sel_gather, it[j].n * fr_bytes);   // (growing synchronises the device)
            if (rc) return rc;
            vt->gather_scalars(st, d_shared, shared_n, it[j].index, it[j].offset, flags + j, it[j].n, (uint32_t *)ctx->sel_gather.p);
            HIP_TRY(ctx, hipGetLastError());
            sc = (const uint32_t *)ctx->sel_gather.p;
        }
        const int rc = msm_device_ranges(ctx, vt, it[j].bases, sc, it[j].n, it[j].out, opts);
        if (rc) return rc;
    }
    return AMDMSM_OK;
}

// argument rules the two batch-items entries share; host_side: the index lists can be read here
int check_batch_items(amdmsm_ctx *ctx, int k, const amdmsm_batch_item *items, const void *shared, size_t shared_n, bool host_side) {
    if (k < 1 || k > MAX_BATCH || !items) return fail(ctx, AMDMSM_ERR_BAD_ARG, "batch of 1 .. 8 MSMs");
    for (int j = 0; j < k; ++j) {
        const amdmsm_batch_item &m = items[j];
        const std::string who = "item " + std::to_string(j) + ": ";
        if (m.struct_size != sizeof(amdmsm_batch_item))
            return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "amdmsm_batch_item.struct_size does not match this library: initialise with AMDMSM_BATCH_ITEM_INIT");
        if (!m.out_xyz || (m.n && !m.bases)) return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "null pointer");
        if (m.n >= ((size_t)1 << 32)) return fail(ctx, AMDMSM_ERR_TOO_LARGE, who + "n must be < 2^32");
        if (m.scalars && m.index) return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "scalars and index are both given");
        if (m.scalars || !m.n) continue;
        if (!shared) return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "scalars == NULL and there is no shared vector");
        if (!m.index) {
            if (m.shared_offset > shared_n || m.n > shared_n - m.shared_offset)
                return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "the slice [shared_offset, shared_offset + n) ends past shared_n");
        } else if (host_side) {
            for (size_t i = 0; i < m.n; ++i) {
                if (m.index[i] >= shared_n)
                    return fail(ctx, AMDMSM_ERR_BAD_ARG, who + "index[" + std::to_string(i) + "] = " + std::to_string(m.index[i]) + " >= shared_n");
            }
        }
    }
    return AMDMSM_OK;
}

// the flags of a finished batch (the stream has been synchronised): the first MSM that named a missing element
int check_batch_flags(amdmsm_ctx *ctx, int k, const uint32_t *h_flags) {
    for (int j = 0; j < k; ++j) {
        if (h_flags[j])
            return fail(ctx, AMDMSM_ERR_BAD_ARG, "item " + std::to_string(j) + ": an index >= shared_n (taken as scalar 0; the results of this batch are void)");
    }
    return AMDMSM_OK;
}

}  // namespace

const group_vtable *amdmsm_internal_find_vt(int curve, int group) { return find_vt(curve, group); }
void *amdmsm_internal_stream(amdmsm_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" {

int amdmsm_abi_version(void) { return AMDMSM_ABI_VERSION; }

int amdmsm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *amdmsm_strerror(int code) {
    switch (code) {
    case AMDMSM_OK: return "ok";
    case AMDMSM_ERR_NO_DEVICE: return "no gfx950 device available (this library has no CPU path)";
    case AMDMSM_ERR_BAD_ARG: return "bad argument";
    case AMDMSM_ERR_UNSUPPORTED: return "unsupported curve/group";
    case AMDMSM_ERR_HIP: return "HIP runtime error";
    case AMDMSM_ERR_TOO_LARGE: return "input too large for one call";
    default: return "unknown error";
    }
}

const char *amdmsm_last_error(const amdmsm_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err_no_ctx.c_str(); }

int amdmsm_ctx_create(int device, amdmsm_ctx **out) {
    if (!out) return AMDMSM_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AMDMSM_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return AMDMSM_ERR_BAD_ARG;
    amdmsm_ctx *ctx = new amdmsm_ctx();
    ctx->device = device;
    dev_guard g(device);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return AMDMSM_ERR_HIP;
    }
    for (auto &e : ctx->ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            delete ctx;
            return AMDMSM_ERR_HIP;
        }
    }
    if (hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->bases_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->host_done, hipEventDisableTiming) != hipSuccess) {
        delete ctx;
        return AMDMSM_ERR_HIP;
    }
    for (auto &set : ctx->ring) {
        for (auto &e : set) {
            if (timing_event(&e) != hipSuccess) {
                delete ctx;
                return AMDMSM_ERR_HIP;
            }
        }
    }
    for (auto &e : ctx->aux_ev) {
        if (timing_event(&e) != hipSuccess) {
            delete ctx;
            return AMDMSM_ERR_HIP;
        }
    }
    for (auto &sl : ctx->slots) {
        bool ok = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) == hipSuccess;
        for (hipEvent_t *e : {&sl.ov_in, &sl.ov_acc, &sl.ov_tail}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        for (auto &e : sl.tail_done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto &e : sl.acc_done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto &q : sl.side) ok = ok && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess;
        if (!ok) {
            delete ctx;
            return AMDMSM_ERR_HIP;
        }
    }
    *out = ctx;
    return AMDMSM_OK;
}

void amdmsm_ctx_destroy(amdmsm_ctx *ctx) {
    if (!ctx) return;
    {
        dev_guard g(ctx->device);
        (void)hipDeviceSynchronize();
        for (auto &sl : ctx->slots) {
            if (sl.ws) (void)hipFree(sl.ws);
            if (sl.done) (void)hipEventDestroy(sl.done);
            for (hipEvent_t e : {sl.ov_in, sl.ov_acc, sl.ov_tail}) {
                if (e) (void)hipEventDestroy(e);
            }
            for (auto &e : sl.acc_done) {
                if (e) (void)hipEventDestroy(e);
            }
            for (auto &e : sl.tail_done) {
                if (e) (void)hipEventDestroy(e);
            }
            for (auto &q : sl.side) {
                if (q) (void)hipStreamDestroy(q);
            }
        }
        for (auto &e : ctx->ev) {
            if (e) (void)hipEventDestroy(e);
        }
        for (auto &set : ctx->ring) {
            for (auto &e : set) {
                if (e) (void)hipEventDestroy(e);
            }
        }
        if (ctx->chunk_partials) (void)hipFree(ctx->chunk_partials);
        if (ctx->seg_host) (void)hipHostFree(ctx->seg_host);
        if (ctx->seg_copied) (void)hipEventDestroy(ctx->seg_copied);
        for (auto &e : ctx->aux_ev) {
            if (e) (void)hipEventDestroy(e);
        }
        for (auto &e : ctx->call_ev) (void)hipEventDestroy(e);
        if (ctx->fb.used) (void)hipEventDestroy(ctx->fb.used);
        for (hipEvent_t e : ctx->fb.uploaded) {
            if (e) (void)hipEventDestroy(e);
        }
        if (ctx->fb.h_up) (void)hipHostFree(ctx->fb.h_up);
        for (auto &t : ctx->fr_tw) {
            if (t.buf.p) (void)hipFree(t.buf.p);
            if (t.ev) (void)hipEventDestroy(t.ev);
        }
        for (fr_matrix *m : ctx->fr_mats) {
            for (void *p : {m->words, m->coef, m->desc, m->lane_rows, m->comb, m->offsets, m->cols})
                if (p) (void)hipFree(p);
            for (auto &u : m->users) (void)hipEventDestroy(u.second);
            delete m;
        }
        for (int b = 0; b < stream_state::NB; ++b) {
            if (ctx->ss.h_stage[b]) (void)hipHostFree(ctx->ss.h_stage[b]);
            if (ctx->ss.streams[b]) (void)hipStreamDestroy(ctx->ss.streams[b]);
        }
        for (grow_buf *b : {&ctx->hb_src, &ctx->hb_aff, &ctx->hb_sc, &ctx->hb_out, &ctx->hb_stats, &ctx->hb_idx, &ctx->sel_flag, &ctx->sel_gather, &ctx->short_word, &ctx->short_out, &ctx->fb.small, &ctx->fb.table,
                            &ctx->fb.table_aff, &ctx->fb.out, &ctx->ss.d_raw[0], &ctx->ss.d_raw[1], &ctx->ss.d_aff[0],
                            &ctx->ss.d_aff[1], &ctx->ss.d_sc[0], &ctx->ss.d_sc[1], &ctx->ss.partials, &ctx->ss.status}) {
            if (b->p) (void)hipFree(b->p);
        }
        for (auto &be : ctx->bases) {
            if (be.d_aff) (void)hipFree(be.d_aff);
            if (be.d_endo) (void)hipFree(be.d_endo);
        }
        if (ctx->bases_ready) (void)hipEventDestroy(ctx->bases_ready);
        if (ctx->host_done) (void)hipEventDestroy(ctx->host_done);
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        if (ctx->bulk_stream) (void)hipStreamDestroy(ctx->bulk_stream);
        if (ctx->tail_stream) (void)hipStreamDestroy(ctx->tail_stream);
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

int amdmsm_sizes(int curve, int group, size_t out[4]) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt || !out) return AMDMSM_ERR_UNSUPPORTED;
    out[0] = (size_t)vt->fr_words * 4;
    out[1] = (size_t)vt->el_words * 3 * 4;
    out[2] = (size_t)vt->el_words * 2 * 4;
    out[3] = (size_t)vt->fr_bits;
    return AMDMSM_OK;
}

int amdmsm_plan_ex(int curve, int group, size_t n, int window_bits, int endomorphism, int *c, int *num_windows,
                   uint32_t *num_buckets, size_t *workspace_bytes, int *endomorphism_used) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return AMDMSM_ERR_UNSUPPORTED;
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    o.window_bits = window_bits;
    o.endomorphism = endomorphism;
    const bool glv = use_endomorphism(vt, n, &o, 0);
    plan_req req;
    req.entries = glv ? 2 * n : n;
    req.c = window_bits;
    req.glv = glv;
    plan_t p;
    const int rc = make_plan(vt, req, p);
    if (rc) return rc;
    if (c) *c = p.c;
    if (num_windows) *num_windows = p.W;
    if (num_buckets) *num_buckets = p.B;
    if (workspace_bytes) *workspace_bytes = p.total;
    if (endomorphism_used) *endomorphism_used = glv ? 1 : 0;
    return AMDMSM_OK;
}

int amdmsm_plan_sort(int curve, int group, size_t n, int window_bits, int endomorphism, size_t out[5]) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt || !out) return AMDMSM_ERR_UNSUPPORTED;
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    o.window_bits = window_bits;
    o.endomorphism = endomorphism;
    const bool glv = use_endomorphism(vt, n, &o, 0);
    plan_req req;
    req.entries = glv ? 2 * n : n;
    req.c = window_bits;
    req.glv = glv;
    plan_t p;
    const int rc = make_plan(vt, req, p);
    if (rc) return rc;
    if (p.c > 22) return AMDMSM_ERR_UNSUPPORTED;
    const sort_geom g = sort_geometry(glv ? 2 * n : n, p.c, p.W);
    out[0] = glv ? 2 * n : n;
    out[1] = (size_t)g.hb;
    out[2] = (size_t)g.fb;
    out[3] = g.chunk_cap;
    out[4] = g.big_thresh;
    return AMDMSM_OK;
}

int amdmsm_plan_sort_digit_grid(size_t items, unsigned block_min, unsigned workgroups, size_t out[3]) {
    if (!out || workgroups == 0) return AMDMSM_ERR_BAD_ARG;
    // the launcher's own function (msm_group.hip l_sort)
    const digit_grid g = sort_digit_grid(items, block_min, workgroups);
    out[0] = g.block;
    out[1] = g.blocks;
    out[2] = g.grid;
    return AMDMSM_OK;
}

int amdmsm_plan_top_window(int curve, int group, size_t n, int window_bits, int endomorphism, int scalars_plain, int out[4]) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt || !out) return AMDMSM_ERR_UNSUPPORTED;
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    o.window_bits = window_bits;
    o.endomorphism = endomorphism;
    const bool glv = use_endomorphism(vt, n, &o, 0);
    plan_req req;
    req.entries = glv ? 2 * n : n;
    req.c = window_bits;
    req.glv = glv;
    plan_t p;
    const int rc = make_plan(vt, req, p);
    if (rc) return rc;
    if (p.c > 22) return AMDMSM_ERR_UNSUPPORTED;
    // the sort launcher's own value (msm_group.hip l_sort asks the same function)
    out[1] = vt->sort_top_window(glv ? 2 : 0, scalars_plain ? 0 : 1, p.c, p.W, glv ? 2 * n : n, &out[0]);
    out[2] = p.c;
    out[3] = p.W;
    return AMDMSM_OK;
}

int amdmsm_plan(int curve, int group, size_t n, int window_bits, int *c, int *num_windows, uint32_t *num_buckets,
                size_t *workspace_bytes) {
    return amdmsm_plan_ex(curve, group, n, window_bits, 0, c, num_windows, num_buckets, workspace_bytes, nullptr);
}

size_t amdmsm_pippenger_optimal_c(size_t num_elements) {
    // multiexp.tcc:35-40 (size_t wrap-around arithmetic kept as is)
    const size_t l = libff_log2(num_elements);
    return l - (l / 3 - 2);
}

size_t amdmsm_bdlo12_signed_optimal_c(size_t num_elements) {
    return amdmsm_pippenger_optimal_c(num_elements) + 1;   // multiexp.tcc:637-641
}

int amdmsm_set_timing(amdmsm_ctx *ctx, int enable) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    ctx->timing = enable != 0;
    for (auto &sl : ctx->slots) sl.ev_valid = false;
    return AMDMSM_OK;
}

int amdmsm_set_pipeline_depth(amdmsm_ctx *ctx, int depth) {
    if (!ctx || depth < 1 || depth > MAX_SLOTS) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    static const bool overlap_wanted = getenv("AMDMSM_OVERLAP") && atoi(getenv("AMDMSM_OVERLAP")) != 0;
    if (depth > 1 && overlap_wanted && !ctx->bulk_stream) {
        // overlap mode's two streams, created when first needed.
        // Both streams need hardware queues of their own: the runtime multiplexes a process's streams over a few
        // hardware queues, and a stream that shares one with a caller's stream sits behind that stream's barrier
        // packets (its wait for the previous MSM's tail) -- seen in kernel traces as a bulk part that starts only after
        // that tail.  Streams created with a CU mask get a dedicated queue (the mask is a queue property); the mask
        // here names every CU.  AMDMSM_STREAM_KIND: 0 plain streams, 1 tails on a high-priority stream, 2 (default)
        // full-CU-mask streams, 3 both high priority (experiments, profiles/r03_experiments.txt).
        static const int kind = getenv("AMDMSM_STREAM_KIND") ? atoi(getenv("AMDMSM_STREAM_KIND")) : 2;
        int least = 0, greatest = 0;
        HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        if (kind == 2) {
            int cus = 256;
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
            std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xffffffffu);
            if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
            HIP_TRY(ctx, hipExtStreamCreateWithCUMask(&ctx->bulk_stream, (uint32_t)mask.size(), mask.data()));
            HIP_TRY(ctx, hipExtStreamCreateWithCUMask(&ctx->tail_stream, (uint32_t)mask.size(), mask.data()));
        } else {
            HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->bulk_stream, hipStreamNonBlocking, kind == 3 ? greatest : 0));
            HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->tail_stream, hipStreamNonBlocking, kind == 0 ? 0 : greatest));
        }
    }
    ctx->depth = depth;
    ctx->next = 0;
    return AMDMSM_OK;
}

int amdmsm_last_slot(amdmsm_ctx *ctx) { return ctx ? ctx->last_slot : AMDMSM_ERR_BAD_ARG; }

int amdmsm_get_timings_by_ticket(amdmsm_ctx *ctx, long long ticket, float ms[AMDMSM_MAX_PHASES]);

int amdmsm_get_slot_timings(amdmsm_ctx *ctx, int slot, float ms[AMDMSM_MAX_PHASES]) {
    if (!ctx || !ms || slot < 0 || slot >= MAX_SLOTS) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    ws_slot &sl = ctx->slots[slot];
    if (!sl.ev_valid) return fail(ctx, AMDMSM_ERR_BAD_ARG, "no timed amdmsm_msm_device call recorded in this slot");
    return amdmsm_get_timings_by_ticket(ctx, sl.last_ticket, ms);
}

long long amdmsm_last_timing_ticket(amdmsm_ctx *ctx) {
    if (!ctx) return -1;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (!ctx->timing || ctx->ticket == 0) return -1;
    return (long long)(ctx->ticket - 1);
}

int amdmsm_get_timings_by_ticket(amdmsm_ctx *ctx, long long ticket, float ms[AMDMSM_MAX_PHASES]) {
    if (!ctx || !ms || ticket < 0) return AMDMSM_ERR_BAD_ARG;
    // under the context lock: no MSM of another thread re-records ring events meanwhile.  The slot of
    // ticket (next - TIMING_RING) is the one the next (or a failed) call records into: not readable.
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    for (int i = 0; i < AMDMSM_MAX_PHASES; ++i) ms[i] = 0.f;
    if ((uint64_t)ticket >= ctx->ticket || ctx->ticket - (uint64_t)ticket >= TIMING_RING)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "timing ticket is not (or no longer) held");
    hipEvent_t *ev = ctx->ring[(uint64_t)ticket % TIMING_RING];
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipEventSynchronize(ev[5]));
    if (ticket == ctx->call_ticket && ctx->call_marks >= 2) {   // a marked call: phases summed over stages and chunks
        const size_t last = ctx->call_marks - 1;
        HIP_TRY(ctx, hipEventSynchronize(ctx->call_ev[last]));
        for (size_t i = 0; i < last; ++i) {
            float d = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&d, ctx->call_ev[i], ctx->call_ev[i + 1]));
            ms[ctx->call_phase[i]] += d;
        }
        HIP_TRY(ctx, hipEventElapsedTime(&ms[AMDMSM_PH_TOTAL], ctx->call_ev[0], ctx->call_ev[last]));
        return AMDMSM_OK;
    }
    for (int i = 0; i < 5; ++i) HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[AMDMSM_PH_TOTAL], ev[0], ev[5]));
    return AMDMSM_OK;
}

int amdmsm_get_timings(amdmsm_ctx *ctx, float ms[AMDMSM_MAX_PHASES]) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    return amdmsm_get_slot_timings(ctx, ctx->last_slot, ms);
}

#define GET_VT(ctx, curve, group)                                         \
    if (!ctx) return AMDMSM_ERR_BAD_ARG;                                  \
    const group_vtable *vt = find_vt(curve, group);                       \
    if (!vt) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group"); \
    std::lock_guard<std::recursive_mutex> lock_(ctx->mu);                           \
    dev_guard guard_(ctx->device)

int amdmsm_msm_device(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, const void *d_scalars,
                      size_t n, void *d_out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (!d_out_xyz || (n && (!d_bases_affine || !d_scalars))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    return msm_device_ranges(ctx, vt, (const uint32_t *)d_bases_affine, (const uint32_t *)d_scalars, n,
                             (uint32_t *)d_out_xyz, opts);
}

int amdmsm_msm_device_batch(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *d_bases_affine,
                            const void *const *d_scalars, size_t n, void *const *d_out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (k < 1 || k > MAX_BATCH || !d_bases_affine || !d_scalars || !d_out_xyz) return fail(ctx, AMDMSM_ERR_BAD_ARG, "batch of 1 .. 8 MSMs");
    for (int j = 0; j < k; ++j) {
        if (!d_out_xyz[j] || (n && (!d_bases_affine[j] || !d_scalars[j]))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    }
    // one MSM, an empty one, or one too long for a single pass: the MSMs one after the other
    if (k == 1 || n == 0 || n > max_range_points() || (size_t)k * n >= ((size_t)1 << 30)) {
        for (int j = 0; j < k; ++j) {
            const int rc = msm_device_ranges(ctx, vt, (const uint32_t *)d_bases_affine[j], (const uint32_t *)d_scalars[j], n,
                                             (uint32_t *)d_out_xyz[j], opts);
            if (rc) return rc;
        }
        return AMDMSM_OK;
    }
    item_dev it[MAX_BATCH];
    for (int j = 0; j < k; ++j) {
        it[j].bases = (const uint32_t *)d_bases_affine[j];
        it[j].n = n;
        it[j].scalars = (const uint32_t *)d_scalars[j];
        it[j].out = (uint32_t *)d_out_xyz[j];
    }
    return msm_device_batch_items_impl(ctx, vt, k, it, nullptr, 0, nullptr, opts);
}

int amdmsm_msm_device_batch_items(amdmsm_ctx *ctx, int curve, int group, int k, const amdmsm_batch_item *items,
                                  const void *d_shared_scalars, size_t shared_n, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = check_batch_items(ctx, k, items, d_shared_scalars, shared_n, false);
    if (rc) return rc;
    rc = ensure_buf(ctx, ctx->sel_flag, MAX_BATCH * 4);
    if (rc) return rc;
    item_dev it[MAX_BATCH];
    bool indexed = false;
    for (int j = 0; j < k; ++j) {
        it[j].bases = (const uint32_t *)items[j].bases;
        it[j].n = items[j].n;
        it[j].scalars = (const uint32_t *)items[j].scalars;
        it[j].offset = items[j].shared_offset;
        it[j].index = items[j].scalars ? nullptr : items[j].index;
        it[j].out = (uint32_t *)items[j].out_xyz;
        indexed = indexed || (it[j].index && it[j].n);
    }
    rc = run_batch_items(ctx, vt, k, it, (const uint32_t *)d_shared_scalars, shared_n, (uint32_t *)ctx->sel_flag.p, opts);
    if (rc || !indexed) return rc;
    // index lists live in HBM: whether one of them named a missing element is known once the digit passes have run
    hipStream_t st = stream_of(ctx, opts);
    uint32_t h_flags[MAX_BATCH] = {};
    HIP_TRY(ctx, hipMemcpyAsync(h_flags, ctx->sel_flag.p, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return check_batch_flags(ctx, k, h_flags);
}

size_t amdmsm_precompute_num_digits(int curve, size_t c) {
    // multiexp_stream.tcc:205, profile_multiexp.cpp:126: (FieldT::num_bits + c - 1) / c
    const group_vtable *vt = find_vt(curve, AMDMSM_G1);
    if (!vt || c == 0) return 0;
    return ((size_t)vt->fr_bits + c - 1) / c;
}

int amdmsm_precompute_bases_device(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, size_t n,
                                   size_t c, size_t num_digits, void *d_table, void *stream) {
    GET_VT(ctx, curve, group);
    if (c < 2 || c > 22 || num_digits < 1 || num_digits > 512) return fail(ctx, AMDMSM_ERR_BAD_ARG, "c / num_digits");
    if (n && (!d_bases_affine || !d_table)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (!n) return AMDMSM_OK;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const size_t aff_bytes = (size_t)vt->el_words * 8;
    const size_t chunk = std::min(n, (size_t)1 << 18);
    void *tmp = nullptr;
    HIP_TRY(ctx, hipMalloc(&tmp, chunk * num_digits * aff_bytes));
    for (size_t lo = 0; lo < n; lo += chunk) {
        const size_t cnt = std::min(chunk, n - lo);
        vt->precompute_table(st, (const uint32_t *)((const char *)d_bases_affine + lo * aff_bytes), cnt, (int)c,
                             (int)num_digits, (uint32_t *)tmp, (uint32_t *)((char *)d_table + lo * num_digits * aff_bytes));
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    HIP_TRY(ctx, e1);
    HIP_TRY(ctx, e2);
    return AMDMSM_OK;
}

int amdmsm_msm_precomputed_device(amdmsm_ctx *ctx, int curve, int group, const void *d_table, const void *d_scalars,
                                  size_t n, size_t c, size_t num_digits, void *d_out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (!d_out_xyz || (n && (!d_table || !d_scalars))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (c < 2 || c > 22 || num_digits < 1 || num_digits > 512) return fail(ctx, AMDMSM_ERR_BAD_ARG, "c / num_digits");
    // more digits than the scalar has windows (+1 for the final carry) would only index multiples
    // that are never selected; such a table layout is a caller error
    if (num_digits > ((size_t)vt->fr_bits + c - 1) / c + 1) return fail(ctx, AMDMSM_ERR_BAD_ARG, "num_digits exceeds ceil(bits/c) + 1");
    amdmsm_opts o = opts_or_default(opts);
    o.window_bits = (int)c;
    // one sorted list holds n * num_digits entries and is indexed with 31 bits: larger inputs are
    // split into ranges of points whose partial results are summed (multiexp.tcc:663-687 shape)
    // (AMDMSM_TABLE_MAX_ENTRIES lowers the limit so that tests can reach the split path)
    static const size_t max_entries = getenv("AMDMSM_TABLE_MAX_ENTRIES") ? (size_t)atoll(getenv("AMDMSM_TABLE_MAX_ENTRIES"))
                                                                         : ((size_t)1 << 31) - 1;
    const size_t max_pts = std::max<size_t>(1, max_entries / num_digits);
    if (n <= max_pts) {
        return msm_device_impl(ctx, vt, (const uint32_t *)d_table, (const uint32_t *)d_scalars, n, (uint32_t *)d_out_xyz,
                               &o, (int)num_digits);
    }
    const size_t parts = (n + max_pts - 1) / max_pts;
    if (parts > MAX_RANGES) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "input too large for one call");
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    {
        const int rcp = ensure_partials(ctx);
        if (rcp) return rcp;
    }
    const int form = o.out_form;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    hipStream_t st = stream_of(ctx, &o);
    for (size_t k = 0; k < parts; ++k) {
        const size_t lo = k * max_pts, cnt = std::min(max_pts, n - lo);
        const int rc = msm_device_impl(ctx, vt, (const uint32_t *)((const char *)d_table + lo * num_digits * aff_bytes),
                                       (const uint32_t *)((const char *)d_scalars + lo * (size_t)vt->fr_words * 4), cnt,
                                       (uint32_t *)((char *)ctx->chunk_partials + k * xyz_bytes), &o, (int)num_digits);
        if (rc) return rc;
    }
    vt->sum_points(st, (const uint32_t *)ctx->chunk_partials, (int)parts, form, (uint32_t *)d_out_xyz);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));   // the partials buffer is shared by the context
    return AMDMSM_OK;
}

int amdmsm_import_bases_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_xyz, size_t stride_bytes,
                               int base_form, size_t n, void *d_dst_affine, void *stream) {
    GET_VT(ctx, curve, group);
    if (stride_bytes % rec_align(vt) || stride_bytes < (size_t)vt->el_words * 12) return fail(ctx, AMDMSM_ERR_BAD_ARG, "stride");
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    vt->import_bases(st, (const uint32_t *)d_src_xyz, stride_bytes / 4, base_form == AMDMSM_FORM_SPECIAL, n,
                     (uint32_t *)d_dst_affine);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_export_affine_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_affine, size_t n,
                                void *d_dst_xyz, void *stream) {
    GET_VT(ctx, curve, group);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    vt->export_affine(st, (const uint32_t *)d_src_affine, n, (uint32_t *)d_dst_xyz);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_sum_points_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_jacobian, int k,
                             int out_form, void *d_out_xyz, void *stream) {
    GET_VT(ctx, curve, group);
    if (k < 0 || !d_out_xyz) return fail(ctx, AMDMSM_ERR_BAD_ARG, "k");
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    vt->sum_points(st, (const uint32_t *)d_points_jacobian, k, out_form, (uint32_t *)d_out_xyz);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_gen_bases_seq_device(amdmsm_ctx *ctx, int curve, int group, uint64_t first, size_t n, void *d_dst_affine,
                                void *stream) {
    GET_VT(ctx, curve, group);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    vt->gen_bases_seq(st, first, n, (uint32_t *)d_dst_affine);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_field_op_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_a, const void *d_b,
                           void *d_out, size_t n) {
    GET_VT(ctx, curve, group);
    vt->field_op(ctx->stream, op, (const uint32_t *)d_a, (const uint32_t *)d_b, (uint32_t *)d_out, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_field_probe_device(amdmsm_ctx *ctx, int curve, int group, int impl, int op, const void *d_a, const void *d_b,
                              const void *d_c, const void *d_d, void *d_out, uint32_t *d_flag, size_t n) {
    GET_VT(ctx, curve, group);
    if ((impl != 0 && impl != 1) || !d_a || !d_out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "impl / operands");
    const bool known = (op >= FPROBE_MUL && op <= FPROBE_SQRT) || (op >= FPROBE_MUL_LZ && op <= FPROBE_CANON);
    if (!known) return fail(ctx, AMDMSM_ERR_BAD_ARG, "op");
    const int arity = op == FPROBE_MUL_SUB_MUL_LZ ? 4
                      : (op == FPROBE_MUL || op == FPROBE_ADD || op == FPROBE_SUB || op == FPROBE_CNEG || op == FPROBE_MUL_LZ ||
                         op == FPROBE_SUB_LZ || op == FPROBE_ADD_LZ) ? 2 : 1;
    if ((arity >= 2 && !d_b) || (arity == 4 && (!d_c || !d_d))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "missing operand");
    vt->field_probe(ctx->stream, impl, op, (const uint32_t *)d_a, (const uint32_t *)d_b, (const uint32_t *)d_c,
                    (const uint32_t *)d_d, (uint32_t *)d_out, d_flag, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_xyzz_probe_device(amdmsm_ctx *ctx, int curve, int group, int impl, int op, const void *d_acc, const void *d_pt,
                             void *d_out, size_t n) {
    GET_VT(ctx, curve, group);
    if ((impl != 0 && impl != 1) || !d_acc || !d_out || op < XPROBE_MADD_LZ || op > XPROBE_TO_JAC)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "impl / op / operands");
    const bool needs_pt = op == XPROBE_MADD_LZ || op == XPROBE_MADD || op == XPROBE_ADD || op == XPROBE_DBL_AFFINE;
    if (needs_pt && !d_pt) return fail(ctx, AMDMSM_ERR_BAD_ARG, "missing operand");
    vt->xyzz_probe(ctx->stream, impl, op, (const uint32_t *)d_acc, (const uint32_t *)d_pt, (uint32_t *)d_out, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

// "<curve>_g<group>" for the message of a probe the group's unit does not carry
static std::string probe_group_name(int curve, int group) {
    static const char *const names[] = {"alt_bn128", "bls12_377", "bw6_761", "bls12_381", "mnt4", "mnt6"};
    const std::string c = curve >= 0 && curve < 6 ? names[curve] : "curve " + std::to_string(curve);
    return c + "_g" + std::to_string(group);
}

int amdmsm_rr_probe_device(amdmsm_ctx *ctx, int curve, int group, int op, int k, const void *d_a, const void *d_b,
                           const void *d_c, const void *d_d, const void *d_w, void *d_out, void *d_outw, uint32_t *d_flag,
                           size_t n) {
    GET_VT(ctx, curve, group);
    if (!vt->rr_probe)
        return fail(ctx, AMDMSM_ERR_UNSUPPORTED, probe_group_name(curve, group) + " does not use the reduced-radix layer");
    const bool known = (op >= RRPROBE_MUL && op <= RRPROBE_EXPORT_D) || (op >= RRPROBE_NORM && op <= RRPROBE_SET_POW2_BL_D);
    if (!known) return fail(ctx, AMDMSM_ERR_BAD_ARG, "op");
    if (!d_out || !d_outw || !d_flag) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null output");
    if (op == RRPROBE_SMALL_TIMES && (k < 2 || k > 4)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "k");
    if (op == RRPROBE_FIRST_REDUCED && !vt->rr_probe_first_reduced)
        return fail(ctx, AMDMSM_ERR_UNSUPPORTED, probe_group_name(curve, group) + " has no table for the reduced first point");
    const bool words_in = op == RRPROBE_FROM_WORDS_RHO || (op >= RRPROBE_FROM_WORDS_0 && op <= RRPROBE_FIRST_COORD);
    const bool none_in = op == RRPROBE_SET_POW2_BL || op == RRPROBE_SET_POW2_BL_D;
    const int arity = (op == RRPROBE_MUL2 || op == RRPROBE_RE_MUL_SUB_MUL) ? 4 : (op == RRPROBE_MUL || op == RRPROBE_RE_MUL) ? 2 : 1;
    if (words_in ? !d_w : (!none_in && (!d_a || (arity >= 2 && !d_b) || (arity == 4 && (!d_c || !d_d)))))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "missing operand");
    vt->rr_probe(ctx->stream, op, k, (const int32_t *)d_a, (const int32_t *)d_b, (const int32_t *)d_c, (const int32_t *)d_d,
                 (const uint32_t *)d_w, (int32_t *)d_out, (uint32_t *)d_outw, d_flag, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_xyzz_rr_probe_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_acc, const void *d_sec,
                                const void *d_pt, const uint32_t *d_fin, void *d_out, void *d_outw, uint32_t *d_fout, size_t n) {
    GET_VT(ctx, curve, group);
    if (!vt->xyzz_rr_probe)
        return fail(ctx, AMDMSM_ERR_UNSUPPORTED, probe_group_name(curve, group) + " does not use the reduced-radix layer");
    const bool known = (op >= XRRPROBE_MADD && op <= XRRPROBE_EXPORT_RHO) || op == XRRPROBE_DBL_RHO || op == XRRPROBE_ADD_RHO ||
                       (op >= XRRPROBE_JAC_DBL && op <= XRRPROBE_JAC_IS_INF);
    if (!known) return fail(ctx, AMDMSM_ERR_BAD_ARG, "op");
    if (!d_acc || !d_out || !d_outw || !d_fout) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null accumulator / output");
    if (((op == XRRPROBE_MADD || op == XRRPROBE_FIRST) && !d_pt) || ((op == XRRPROBE_ADD_RHO || op == XRRPROBE_JAC_MADD) && !d_sec))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "missing operand");
    vt->xyzz_rr_probe(ctx->stream, op, (const int32_t *)d_acc, (const int32_t *)d_sec, (const uint32_t *)d_pt, d_fin,
                      (int32_t *)d_out, (uint32_t *)d_outw, d_fout, n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_group_op_device(amdmsm_ctx *ctx, int curve, int group, int op, const void *d_a, const void *d_b,
                           void *d_out, size_t n, int out_form) {
    GET_VT(ctx, curve, group);
    vt->group_op(ctx->stream, op, (const uint32_t *)d_a, (const uint32_t *)d_b, (uint32_t *)d_out, n, out_form);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_digits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n, int scalars_plain,
                         int c, int num_windows, int32_t *d_out) {
    GET_VT(ctx, curve, group);
    if (c < 2 || c > 24 || num_windows < 1) return fail(ctx, AMDMSM_ERR_BAD_ARG, "c / num_windows");
    vt->digits(ctx->stream, (const uint32_t *)d_scalars, n, scalars_plain ? 0 : 1, c, num_windows, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_endomorphism_digits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n,
                                      int scalars_plain, int c, int num_windows, int32_t *d_out) {
    GET_VT(ctx, curve, group);
    if (!vt->has_endomorphism) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "the group has no endomorphism");
    if (c < 2 || c > 24 || num_windows < 1) return fail(ctx, AMDMSM_ERR_BAD_ARG, "c / num_windows");
    vt->glv_digits(ctx->stream, (const uint32_t *)d_scalars, n, scalars_plain ? 0 : 1, c, num_windows, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_endomorphism_info(int curve, int group, void *lambda_plain, int *bound_log2_x1000, int *prime_order) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt || !vt->has_endomorphism) return AMDMSM_ERR_UNSUPPORTED;
    if (lambda_plain) memcpy(lambda_plain, vt->glv_lambda, (size_t)vt->fr_words * 4);
    if (bound_log2_x1000) *bound_log2_x1000 = vt->glv_bound_log2_x1000;
    if (prime_order) *prime_order = vt->prime_order;
    return AMDMSM_OK;
}

int amdmsm_mul_bench_device(amdmsm_ctx *ctx, int curve, int group, void *d_inout, size_t nthreads, int iters,
                            int inline_variant, float *ms) {
    GET_VT(ctx, curve, group);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[AMDMSM_MAX_PHASES - 1], ctx->stream));
    vt->mul_bench(ctx->stream, (uint32_t *)d_inout, nthreads, iters, inline_variant);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[AMDMSM_MAX_PHASES], ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[AMDMSM_MAX_PHASES]));
    if (ms) HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev[AMDMSM_MAX_PHASES - 1], ctx->ev[AMDMSM_MAX_PHASES]));
    return AMDMSM_OK;
}

int amdmsm_madd_bench_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, void *d_out_xyz,
                             size_t nthreads, int iters, int inline_variant, float *ms) {
    GET_VT(ctx, curve, group);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[AMDMSM_MAX_PHASES - 1], ctx->stream));
    vt->madd_bench(ctx->stream, (const uint32_t *)d_points_affine, (uint32_t *)d_out_xyz, nthreads, iters,
                   inline_variant);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[AMDMSM_MAX_PHASES], ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[AMDMSM_MAX_PHASES]));
    if (ms) HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev[AMDMSM_MAX_PHASES - 1], ctx->ev[AMDMSM_MAX_PHASES]));
    return AMDMSM_OK;
}

int amdmsm_malloc(amdmsm_ctx *ctx, size_t bytes, void **d_ptr) {
    if (!ctx || !d_ptr) return AMDMSM_ERR_BAD_ARG;
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipMalloc(d_ptr, bytes ? bytes : 16));
    return AMDMSM_OK;
}

int amdmsm_free(amdmsm_ctx *ctx, void *d_ptr) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipFree(d_ptr));
    return AMDMSM_OK;
}

int amdmsm_memcpy_h2d(amdmsm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_memcpy_d2h(amdmsm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return AMDMSM_OK;
}

int amdmsm_synchronize(amdmsm_ctx *ctx) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    return AMDMSM_OK;
}

// ------------------------------------------------------------ host entries
}   // extern "C"

namespace {

int ensure_buf(amdmsm_ctx *ctx, grow_buf &b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return AMDMSM_OK;
    if (b.p) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t want = std::max<size_t>(bytes + bytes / 8, 256);
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    return AMDMSM_OK;
}

// resident compact-affine copy of the host range [bases, bases + n*stride), or null
void *find_resident_bases(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases, size_t stride, int form, size_t n,
                          base_entry **entry = nullptr, size_t *first = nullptr) {
    const char *lo = (const char *)bases;
    for (auto &e : ctx->bases) {
        if (e.curve != vt->curve || e.group != vt->group || e.form != form || e.stride != stride) continue;
        if (lo < e.host || lo + n * stride > e.host + e.n * e.stride) continue;
        const size_t off = (size_t)(lo - e.host);
        if (off % stride) continue;
        e.last_use = ++ctx->use_clock;
        if (entry) *entry = &e;
        if (first) *first = off / stride;
        return (char *)e.d_aff + (off / stride) * (size_t)vt->el_words * 8;
    }
    return nullptr;
}

int register_bases_impl(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases, size_t stride, int form, size_t n,
                        bool automatic, uint64_t *handle) {
    const size_t aff_bytes = (size_t)vt->el_words * 8;
    base_entry e;
    e.curve = vt->curve;
    e.group = vt->group;
    e.form = form;
    e.host = (const char *)bases;
    e.n = n;
    e.stride = stride;
    e.automatic = automatic;
    e.aff_bytes = aff_bytes;
    HIP_TRY(ctx, hipMalloc(&e.d_aff, std::max<size_t>(n * aff_bytes, 256)));
    int rc = ensure_buf(ctx, ctx->hb_src, n * stride);
    if (rc == AMDMSM_OK) {
        hipError_t he = hipMemcpyAsync(ctx->hb_src.p, bases, n * stride, hipMemcpyHostToDevice, ctx->stream);
        if (he == hipSuccess) {
            vt->import_bases(ctx->stream, (const uint32_t *)ctx->hb_src.p, stride / 4, form == AMDMSM_FORM_SPECIAL, n,
                             (uint32_t *)e.d_aff);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
        if (he != hipSuccess) rc = fail(ctx, AMDMSM_ERR_HIP, std::string("register_bases: ") + hipGetErrorString(he));
    }
    if (rc) {
        (void)hipFree(e.d_aff);
        return rc;
    }
    e.id = ctx->next_base_id++;
    e.last_use = ++ctx->use_clock;
    ctx->bases.push_back(e);
    if (handle) *handle = e.id;
    return AMDMSM_OK;
}

// AMDMSM_BASE_CACHE_MB=<cap>: host-buffer calls register the base vectors they see (keyed on
// pointer, length, stride and form) up to <cap> MiB of HBM, least recently used first out.
// Off by default: the caller must not modify a cached vector in place without
// amdmsm_invalidate_bases (the reference re-reads the bases on every call).
size_t auto_cache_cap_bytes() {
    static const size_t cap = getenv("AMDMSM_BASE_CACHE_MB") ? (size_t)atoll(getenv("AMDMSM_BASE_CACHE_MB")) << 20 : 0;
    return cap;
}

void drop_entry(amdmsm_ctx *ctx, size_t i) {
    if (ctx->bases[i].d_aff) (void)hipFree(ctx->bases[i].d_aff);
    if (ctx->bases[i].d_endo) (void)hipFree(ctx->bases[i].d_endo);
    ctx->bases.erase(ctx->bases.begin() + (long)i);
}

void *auto_cache_bases(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases, size_t stride, int form, size_t n) {
    // (an entry is charged twice its affine bytes: the phi(P) records a split MSM attaches later count too)
    const size_t cap = auto_cache_cap_bytes(), need = 2 * n * (size_t)vt->el_words * 8;
    if (!cap || need > cap || n < 1024) return nullptr;
    (void)hipStreamSynchronize(ctx->stream);
    for (;;) {
        size_t used = 0, lru = (size_t)-1;
        for (size_t i = 0; i < ctx->bases.size(); ++i) {
            const base_entry &e = ctx->bases[i];
            if (!e.automatic) continue;
            used += 2 * e.n * e.aff_bytes;
            if (e.pinned) continue;   // a vector the running batch already resolved: its device copy must outlive the call
            if (lru == (size_t)-1 || e.last_use < ctx->bases[lru].last_use) lru = i;
        }
        if (used + need <= cap) break;
        if (lru == (size_t)-1) return nullptr;   // what is left is pinned by the running call: no room, the caller uploads
        drop_entry(ctx, lru);
    }
    if (register_bases_impl(ctx, vt, bases, stride, form, n, true, nullptr) != AMDMSM_OK) return nullptr;
    return ctx->bases.back().d_aff;
}

struct bases_upload {
    amdmsm_ctx *ctx;
    const group_vtable *vt;
    const void *bases;
    size_t stride, n;
    int form;
};
// runs once the sort is enqueued: bases H2D + import on the copy stream (msm_hook)
int upload_bases_hook(void *arg, hipEvent_t *wait_for) {
    bases_upload &u = *(bases_upload *)arg;
    amdmsm_ctx *ctx = u.ctx;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_src.p, u.bases, u.n * u.stride, hipMemcpyHostToDevice, ctx->copy_stream));
    u.vt->import_bases(ctx->copy_stream, (const uint32_t *)ctx->hb_src.p, u.stride / 4, u.form == AMDMSM_FORM_SPECIAL, u.n,
                       (uint32_t *)ctx->hb_aff.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->bases_ready, ctx->copy_stream));
    *wait_for = ctx->bases_ready;
    return AMDMSM_OK;
}

// One MSM over host vectors, enqueued on the context stream; the result is left in
// ctx->hb_out (and the scalar statistics in ctx->hb_stats) -- the caller copies it back.
// Device buffers are the context's grow-only staging buffers: no allocation in steady state.
int host_msm_enqueue(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases_xyz, size_t stride, int base_form,
                     const void *scalars, size_t n, const amdmsm_opts *opts, bool want_stats, bool clear_stats = true,
                     const short_spec *ss = nullptr) {
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    const size_t fr_bytes = ss ? ss->elem_bytes(vt) : (size_t)vt->fr_words * 4;   // packed integers: n * width bytes cross PCIe
    hipStream_t st = ctx->stream;
    int rc = ensure_buf(ctx, ctx->hb_out, xyz_bytes);
    if (rc) return rc;
    if (want_stats) {
        rc = ensure_buf(ctx, ctx->hb_stats, 16);
        if (rc) return rc;
        if (clear_stats) HIP_TRY(ctx, hipMemsetAsync(ctx->hb_stats.p, 0, 16, st));
    }
    amdmsm_opts o = opts_or_default(opts);
    o.stream = st;
    void *d_aff = nullptr;
    const uint32_t *d_endo = nullptr;
    bases_upload up{ctx, vt, bases_xyz, stride, n, base_form};
    msm_hook hook;
    if (n) {
        rc = ensure_buf(ctx, ctx->hb_sc, n * fr_bytes);
        if (rc) return rc;
        base_entry *be = nullptr;
        size_t first = 0;
        d_aff = find_resident_bases(ctx, vt, bases_xyz, stride, base_form, n, &be, &first);
        if (!d_aff && auto_cache_bases(ctx, vt, bases_xyz, stride, base_form, n))
            d_aff = find_resident_bases(ctx, vt, bases_xyz, stride, base_form, n, &be, &first);
        if (d_aff && be && !ss && use_endomorphism(vt, n, &o, 0)) {
            // resident bases keep their phi(P) records too: built once (whole vector), then every
            // split MSM over them skips k_endo_points
            if (!be->d_endo) {
                if (hipMalloc(&be->d_endo, std::max<size_t>(be->n * aff_bytes, 256)) == hipSuccess) {
                    vt->endo_points(st, (const uint32_t *)be->d_aff, be->n, (uint32_t *)be->d_endo);
                    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                        (void)hipFree(be->d_endo);
                        be->d_endo = nullptr;
                    }
                } else {
                    be->d_endo = nullptr;   // no room: the per-call kernel does it
                    (void)hipGetLastError();
                }
            }
            if (be->d_endo) d_endo = (const uint32_t *)((const char *)be->d_endo + first * aff_bytes);
        }
        if (!d_aff) {
            rc = ensure_buf(ctx, ctx->hb_src, n * stride);
            if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, n * aff_bytes);
            if (rc) return rc;
            d_aff = ctx->hb_aff.p;
            hook.fn = upload_bases_hook;
            hook.arg = &up;
        }
        if (!(ss && ss->uploaded)) HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, scalars, n * fr_bytes, hipMemcpyHostToDevice, st));
        if (want_stats) {
            vt->scalar_stats(st, (const uint32_t *)ctx->hb_sc.p, n, o.scalars_plain ? 0 : 1, (uint32_t *)ctx->hb_stats.p);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    return msm_device_impl(ctx, vt, (const uint32_t *)d_aff, (const uint32_t *)ctx->hb_sc.p, n, (uint32_t *)ctx->hb_out.p, &o,
                           0, &hook, d_endo, ss);
}

// one partial point from the device that produced it to the combining device (xGMI peer copy)
// (AMDMSM_FORCE_PEER_COPY=1: the peer-copy call also between two contexts of ONE device, so that a
// one-GPU test box executes the exchange branch of the multi-device entries)
hipError_t copy_partial(hipStream_t st, void *dst, int dst_dev, const void *src, int src_dev, size_t bytes) {
    static const bool force_peer = getenv("AMDMSM_FORCE_PEER_COPY") && atoi(getenv("AMDMSM_FORCE_PEER_COPY")) != 0;
    if (dst_dev == src_dev && !force_peer) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}

// host_msm_enqueue for inputs of any length: above max_range_points() the reference's chunk loop
// (multiexp.tcc:655-687), range after range through the same staging buffers (each range is
// finished before the next one reuses them), the partial points summed at the end.  The result is
// left in ctx->hb_out in the requested form, the 0 / 1 counters of all ranges in ctx->hb_stats.
int host_msm_ranges(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases_xyz, size_t stride, int base_form,
                    const void *scalars, size_t n, const amdmsm_opts *opts, bool want_stats, const short_spec *ss = nullptr) {
    const size_t maxr = max_range_points();
    if (n <= maxr) return host_msm_enqueue(ctx, vt, bases_xyz, stride, base_form, scalars, n, opts, want_stats, true, ss);
    const size_t parts = (n + maxr - 1) / maxr;
    if (parts > MAX_RANGES) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "input too large for one call");
    const size_t one = (n + parts - 1) / parts;   // <= maxr (see msm_device_ranges)
    const size_t xyz_bytes = (size_t)vt->el_words * 12, fr_bytes = ss ? ss->elem_bytes(vt) : (size_t)vt->fr_words * 4;
    short_spec ss_range;   // a range brings its own scalars in
    if (ss) {
        ss_range = *ss;
        ss_range.uploaded = false;
        ss = &ss_range;
    }
    int rc = ensure_partials(ctx);
    if (rc) return rc;
    amdmsm_opts o = opts_or_default(opts);
    const int form = o.out_form;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    hipStream_t st = ctx->stream;
    for (size_t k = 0; k < parts; ++k) {
        const size_t lo = k * one, cnt = (k == parts - 1) ? n - lo : one;
        rc = host_msm_enqueue(ctx, vt, (const char *)bases_xyz + lo * stride, stride, base_form,
                              (const char *)scalars + lo * fr_bytes, cnt, &o, want_stats, k == 0, ss);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync((char *)ctx->chunk_partials + k * xyz_bytes, ctx->hb_out.p, xyz_bytes,
                                    hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    }
    vt->sum_points(st, (const uint32_t *)ctx->chunk_partials, (int)parts, form, (uint32_t *)ctx->hb_out.p);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int check_host_args(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases_xyz, size_t &stride, const void *scalars,
                    size_t n, const void *out_xyz) {
    if (!out_xyz || (n && (!bases_xyz || !scalars))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    if (stride == 0) stride = xyz_bytes;
    if (stride % rec_align(vt) || stride < xyz_bytes) return fail(ctx, AMDMSM_ERR_BAD_ARG, "base stride");
    return AMDMSM_OK;
}

int host_multi_exp(amdmsm_ctx *ctx, const group_vtable *vt, const void *bases_xyz, size_t stride, int base_form,
                   const void *scalars, size_t n, void *out_xyz, const amdmsm_opts *opts, size_t stats[3],
                   const short_spec *ss = nullptr) {
    int rc = check_host_args(ctx, vt, bases_xyz, stride, scalars, n, out_xyz);
    if (rc) return rc;
    rc = host_msm_ranges(ctx, vt, bases_xyz, stride, base_form, scalars, n, opts, stats != nullptr, ss);
    if (rc) {
        (void)hipDeviceSynchronize();   // nothing of this call may still touch the staging buffers
        return rc;
    }
    hipStream_t st = ctx->stream;
    uint32_t hs[4] = {};
    if (ss && ss->flag) {
        // a promise was tested by the digit passes: the result reaches the caller's buffer only if it was kept
        uint32_t raised = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&raised, ss->flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
        if (raised) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a scalar is not below 2^bits (amdmsm_scalar_desc.bits is a promise)");
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, ctx->hb_out.p, (size_t)vt->el_words * 12, hipMemcpyDeviceToHost, st));
    if (stats) HIP_TRY(ctx, hipMemcpyAsync(hs, ctx->hb_stats.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    if (stats) {
        stats[0] = hs[0];
        stats[1] = hs[1];
        stats[2] = n - hs[0] - hs[1];
    }
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_multi_exp(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                     int base_form, const void *scalars, size_t n, void *out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    return host_multi_exp(ctx, vt, bases_xyz, base_stride_bytes, base_form, scalars, n, out_xyz, opts, nullptr);
}

// ---- scalars known to be short -------------------------------------------------------------------------------------
}   // extern "C"

namespace {

// How a call whose scalars are below 2^bits runs.  The endomorphism split is kept only where today's rule would use it
// AND bits exceeds the split's own bound on |k1|, |k2| -- below that bound the split cannot shorten anything and the
// plain path with windows for bits + 2 bits is taken.  bits at or above Fr::num_bits is the ordinary plan.
enum short_route { ROUTE_ORDINARY = 0, ROUTE_SHORT = 1 };
short_route route_short(const group_vtable *vt, size_t n, const amdmsm_opts *opts, int kind, int bits) {
    if (kind != AMDMSM_SCALAR_FR) return ROUTE_SHORT;   // packed integers have no full-width digit pass; 64 bits are below every bound
    if (bits >= vt->fr_bits) return ROUTE_ORDINARY;
    if (bits * 1000 > vt->glv_bound_log2_x1000 && use_endomorphism(vt, n, opts, 0)) return ROUTE_ORDINARY;
    return ROUTE_SHORT;
}

int kind_width_bits(const group_vtable *vt, int kind) { return kind == AMDMSM_SCALAR_FR ? vt->fr_bits : 8 * kind; }

// argument rules of the short entries; *bits_full = the kind's full width
int check_short_args(amdmsm_ctx *ctx, const group_vtable *vt, const amdmsm_scalar_desc *desc, const void *scalars, size_t n,
                     const amdmsm_opts *opts) {
    if (!desc) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null amdmsm_scalar_desc");
    if (desc->struct_size != sizeof(amdmsm_scalar_desc))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "amdmsm_scalar_desc.struct_size does not match this library: initialise with AMDMSM_SCALAR_DESC_INIT");
    const int k = desc->kind;
    if (k != AMDMSM_SCALAR_FR && k != AMDMSM_SCALAR_U8 && k != AMDMSM_SCALAR_U16 && k != AMDMSM_SCALAR_U32 && k != AMDMSM_SCALAR_U64)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "amdmsm_scalar_desc.kind is not an AMDMSM_SCALAR_* value");
    if (desc->bits < -1 || desc->bits > kind_width_bits(vt, k))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "amdmsm_scalar_desc.bits must be -1, 0 or 1 .. the kind's width");
    if (opts && opts->window_bits > 22) return fail(ctx, AMDMSM_ERR_BAD_ARG, "window_bits > 22 is not available for short scalars");
    if (opts && (opts->window_bits < 0 || opts->window_bits == 1)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "bad window_bits");
    if (k != AMDMSM_SCALAR_FR && n && ((uintptr_t)scalars % (uintptr_t)k))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "scalars must be aligned to the element width");
    return AMDMSM_OK;
}

// bit length of the longest of n device-resident scalars, added to what *acc (device word) already holds
int measure_enqueue(amdmsm_ctx *ctx, const group_vtable *vt, const void *d_scalars, int kind, size_t n, int mont, uint32_t *acc,
                    hipStream_t st) {
    vt->scalar_bits(st, d_scalars, kind, n, mont, acc);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int read_word(amdmsm_ctx *ctx, const uint32_t *d_word, hipStream_t st, uint32_t *out) {
    HIP_TRY(ctx, hipMemcpyAsync(out, d_word, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return AMDMSM_OK;
}

int scalar_bits_device_impl(amdmsm_ctx *ctx, const group_vtable *vt, const void *d_scalars, int kind, size_t n, int mont,
                            hipStream_t st, int *bits) {
    int rc = ensure_buf(ctx, ctx->short_word, 8);
    if (rc) return rc;
    uint32_t *acc = (uint32_t *)ctx->short_word.p + 1;
    HIP_TRY(ctx, hipMemsetAsync(acc, 0, 4, st));
    rc = measure_enqueue(ctx, vt, d_scalars, kind, n, mont, acc, st);
    if (rc) return rc;
    uint32_t v = 0;
    rc = read_word(ctx, acc, st, &v);
    if (rc) return rc;
    *bits = (int)v;
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_plan_short(int curve, int group, size_t n, int window_bits, int endomorphism, int scalar_bits, int *c,
                      int *num_windows, uint32_t *num_buckets, size_t *workspace_bytes, int *endomorphism_used) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return AMDMSM_ERR_UNSUPPORTED;
    if (scalar_bits < 0 || window_bits > 22) return AMDMSM_ERR_BAD_ARG;
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    o.window_bits = window_bits;
    o.endomorphism = endomorphism;
    if (scalar_bits == 0 || route_short(vt, n, &o, AMDMSM_SCALAR_FR, scalar_bits) == ROUTE_ORDINARY)
        return amdmsm_plan_ex(curve, group, n, window_bits, endomorphism, c, num_windows, num_buckets, workspace_bytes,
                              endomorphism_used);
    plan_req req;
    req.entries = n;
    req.c = window_bits;
    req.sbits = scalar_bits;
    plan_t p;
    const int rc = make_plan(vt, req, p);
    if (rc) return rc;
    if (c) *c = p.c;
    if (num_windows) *num_windows = p.W;
    if (num_buckets) *num_buckets = p.B;
    if (workspace_bytes) *workspace_bytes = p.total;
    if (endomorphism_used) *endomorphism_used = 0;
    return AMDMSM_OK;
}

int amdmsm_scalar_bits_device(amdmsm_ctx *ctx, int curve, int group, const void *d_scalars, size_t n,
                              const amdmsm_scalar_desc *desc, int scalars_plain, int *bits) {
    GET_VT(ctx, curve, group);
    int rc = check_short_args(ctx, vt, desc, d_scalars, n, nullptr);
    if (rc) return rc;
    if (!bits || (n && !d_scalars)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    return scalar_bits_device_impl(ctx, vt, d_scalars, desc->kind, n, scalars_plain ? 0 : 1, ctx->stream, bits);
}

int amdmsm_msm_device_short(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, const void *d_scalars,
                            const amdmsm_scalar_desc *desc, size_t n, void *d_out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = check_short_args(ctx, vt, desc, d_scalars, n, opts);
    if (rc) return rc;
    if (!d_out_xyz || (n && (!d_bases_affine || !d_scalars))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    hipStream_t st = stream_of(ctx, opts);
    const int kind = desc->kind, full = kind_width_bits(vt, kind);
    const int mont = (opts && opts->scalars_plain) ? 0 : 1;
    const uint32_t *bases = (const uint32_t *)d_bases_affine;
    uint32_t *out = (uint32_t *)d_out_xyz;
    if (n == 0 || (kind == AMDMSM_SCALAR_FR && (desc->bits == 0 || desc->bits >= full)))
        return msm_device_ranges(ctx, vt, bases, (const uint32_t *)d_scalars, n, out, opts);
    int bits = desc->bits ? desc->bits : full;
    bool promise = desc->bits > 0 && desc->bits < full;
    if (desc->bits == -1) {
        rc = scalar_bits_device_impl(ctx, vt, d_scalars, kind, n, mont, st, &bits);
        if (rc) return rc;
        if (bits == 0) return msm_device_impl(ctx, vt, bases, nullptr, 0, out, opts);   // every scalar is zero: the group's zero, no plan
    }
    if (route_short(vt, n, opts, kind, bits) == ROUTE_ORDINARY) {
        // the split (or the full-width plan) serves this length: the ordinary digit pass, which tests nothing -- a
        // promise is checked by the measuring pass before anything else is launched
        if (promise) {
            int longest = 0;
            rc = scalar_bits_device_impl(ctx, vt, d_scalars, kind, n, mont, st, &longest);
            if (rc) return rc;
            if (longest > bits) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a scalar is not below 2^bits (amdmsm_scalar_desc.bits is a promise)");
        }
        return msm_device_ranges(ctx, vt, bases, (const uint32_t *)d_scalars, n, out, opts);
    }
    short_spec ss;
    ss.kind = kind;
    ss.bits = bits;
    if (!promise) return msm_device_ranges(ctx, vt, bases, (const uint32_t *)d_scalars, n, out, opts, &ss);   // asynchronous
    // a promise: the digit pass tests it, and the result is held back until the flag has been read
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    rc = ensure_buf(ctx, ctx->short_word, 8);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->short_out, xyz_bytes);
    if (rc) return rc;
    ss.flag = (uint32_t *)ctx->short_word.p;
    HIP_TRY(ctx, hipMemsetAsync(ss.flag, 0, 4, st));
    rc = msm_device_ranges(ctx, vt, bases, (const uint32_t *)d_scalars, n, (uint32_t *)ctx->short_out.p, opts, &ss);
    if (rc) return rc;
    uint32_t raised = 0;
    rc = read_word(ctx, ss.flag, st, &raised);
    if (rc) return rc;
    if (raised) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a scalar is not below 2^bits (amdmsm_scalar_desc.bits is a promise)");
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->short_out.p, xyz_bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // the held-back result is the context's
    return AMDMSM_OK;
}

int amdmsm_multi_exp_short(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                           int base_form, const void *scalars, const amdmsm_scalar_desc *desc, size_t n, void *out_xyz,
                           const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = check_short_args(ctx, vt, desc, scalars, n, opts);
    if (rc) return rc;
    size_t stride = base_stride_bytes;
    rc = check_host_args(ctx, vt, bases_xyz, stride, scalars, n, out_xyz);
    if (rc) return rc;
    const int kind = desc->kind, full = kind_width_bits(vt, kind);
    if (n == 0 || (kind == AMDMSM_SCALAR_FR && (desc->bits == 0 || desc->bits >= full)))
        return host_multi_exp(ctx, vt, bases_xyz, stride, base_form, scalars, n, out_xyz, opts, nullptr);
    hipStream_t st = ctx->stream;
    amdmsm_opts o = opts_or_default(opts);
    const int mont = o.scalars_plain ? 0 : 1;
    short_spec ss;
    ss.kind = kind;
    const size_t eb = ss.elem_bytes(vt), maxr = max_range_points();
    int bits = desc->bits ? desc->bits : full;
    const bool promise = desc->bits > 0 && desc->bits < full;
    rc = ensure_buf(ctx, ctx->short_word, 8);
    if (rc) return rc;
    // one bit length for the whole call: measured (bits = -1, or a promise the ordinary digit pass cannot test) over
    // every range before anything is planned; a call of one range keeps the scalars it uploaded for that
    auto measure = [&](int *longest) -> int {
        uint32_t *acc = (uint32_t *)ctx->short_word.p + 1;
        HIP_TRY(ctx, hipMemsetAsync(acc, 0, 4, st));
        for (size_t lo = 0; lo < n; lo += maxr) {
            const size_t cnt = std::min(maxr, n - lo);
            int r = ensure_buf(ctx, ctx->hb_sc, cnt * eb);
            if (r) return r;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, (const char *)scalars + lo * eb, cnt * eb, hipMemcpyHostToDevice, st));
            r = measure_enqueue(ctx, vt, ctx->hb_sc.p, kind, cnt, mont, acc, st);
            if (r) return r;
        }
        uint32_t v = 0;
        const int r = read_word(ctx, acc, st, &v);
        *longest = (int)v;
        return r;
    };
    if (desc->bits == -1) {
        rc = measure(&bits);
        if (rc) return rc;
        if (bits == 0) return host_multi_exp(ctx, vt, bases_xyz, stride, base_form, scalars, 0, out_xyz, opts, nullptr);   // the group's zero
        ss.uploaded = n <= maxr;
    }
    if (route_short(vt, n, &o, kind, bits) == ROUTE_ORDINARY) {
        if (promise) {
            int longest = 0;
            rc = measure(&longest);
            if (rc) return rc;
            if (longest > bits) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a scalar is not below 2^bits (amdmsm_scalar_desc.bits is a promise)");
        }
        return host_multi_exp(ctx, vt, bases_xyz, stride, base_form, scalars, n, out_xyz, opts, nullptr);
    }
    ss.bits = bits;
    if (promise) {
        ss.flag = (uint32_t *)ctx->short_word.p;
        HIP_TRY(ctx, hipMemsetAsync(ss.flag, 0, 4, st));
    }
    return host_multi_exp(ctx, vt, bases_xyz, stride, base_form, scalars, n, out_xyz, opts, nullptr, &ss);
}

int amdmsm_multi_exp_filter_one_zero(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz,
                                     size_t base_stride_bytes, int base_form, const void *scalars, size_t n,
                                     void *out_xyz, const amdmsm_opts *opts, size_t stats[3]) {
    // multiexp.tcc:690-757 separates scalars equal to 0 and 1 before the Pippenger
    // pass.  On the device a zero scalar recodes to all-zero digits (no work) and a
    // one lands in bucket 1 of window 0, so the same kernels compute the same sum;
    // only the three statistics the reference prints need the classification, which
    // k_scalar_stats counts on the device from the scalars already in HBM.
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    return host_multi_exp(ctx, vt, bases_xyz, base_stride_bytes, base_form, scalars, n, out_xyz, opts, stats);
}

}   // extern "C"

namespace {

// Every resident base vector a batch resolves is pinned until the call returns: registering vector j under
// AMDMSM_BASE_CACHE_MB evicts least-recently-used automatic entries (hipFree), which must never be the copy an earlier
// MSM of the same batch is about to read.  A vector that does not fit beside the pinned ones is uploaded like an
// unregistered one.
struct unpin_all {
    amdmsm_ctx *c;
    ~unpin_all() {
        for (auto &e : c->bases) e.pinned = false;
    }
};

// A batch over host vectors, its arguments checked (stride: bytes between base records): scalars over PCIe -- the shared
// vector once, own vectors and index lists per item --, bases from the resident copies where registered
// (amdmsm_register_bases) and uploaded + imported otherwise.
int host_batch_items(amdmsm_ctx *ctx, const group_vtable *vt, int k, const amdmsm_batch_item *items, size_t stride, int base_form,
                     const void *shared_scalars, size_t shared_n, const amdmsm_opts *opts) {
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8, fr_bytes = (size_t)vt->fr_words * 4;
    // staging: [shared | own vectors] in hb_sc, the index lists in hb_idx, imported bases of unregistered vectors in hb_aff
    bool any_shared = false;
    size_t sc_bytes = 0, idx_bytes = 0, max_src = 0;
    for (int j = 0; j < k; ++j) {
        const amdmsm_batch_item &m = items[j];
        if (m.scalars) sc_bytes += align_up(m.n * fr_bytes, 256);
        else if (m.n) any_shared = true;
        if (!m.scalars && m.index) idx_bytes += align_up(m.n * 4, 256);
    }
    const size_t shared_bytes = any_shared ? align_up(shared_n * fr_bytes, 256) : 0;
    hipStream_t st = ctx->stream;
    int rc = ensure_buf(ctx, ctx->hb_out, (size_t)MAX_BATCH * xyz_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_sc, shared_bytes + sc_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_idx, idx_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->sel_flag, MAX_BATCH * 4);
    if (rc) return rc;
    // out-of-range flags exist only for a batch that selects from the shared vector
    uint32_t *flags = any_shared ? (uint32_t *)ctx->sel_flag.p : nullptr;
    item_dev it[MAX_BATCH];
    size_t aff_need = 0;
    unpin_all unpin{ctx};
    for (int j = 0; j < k; ++j) {
        const amdmsm_batch_item &m = items[j];
        it[j].n = m.n;
        if (!m.n) continue;
        base_entry *be = nullptr;
        it[j].bases = (const uint32_t *)find_resident_bases(ctx, vt, m.bases, stride, base_form, m.n, &be);
        if (!it[j].bases && auto_cache_bases(ctx, vt, m.bases, stride, base_form, m.n))
            it[j].bases = (const uint32_t *)find_resident_bases(ctx, vt, m.bases, stride, base_form, m.n, &be);
        if (it[j].bases && be) be->pinned = true;
        if (!it[j].bases) {
            aff_need += align_up(m.n * aff_bytes, 256);
            max_src = std::max(max_src, m.n * stride);
        }
    }
    if (aff_need) {
        rc = ensure_buf(ctx, ctx->hb_src, max_src);
        if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, aff_need);
        if (rc) return rc;
    }
    if (any_shared) HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, shared_scalars, shared_n * fr_bytes, hipMemcpyHostToDevice, st));
    size_t sc_off = shared_bytes, idx_off = 0, aff_off = 0;
    for (int j = 0; j < k; ++j) {
        const amdmsm_batch_item &m = items[j];
        it[j].out = (uint32_t *)((char *)ctx->hb_out.p + (size_t)j * xyz_bytes);
        if (!m.n) continue;
        if (m.scalars) {
            it[j].scalars = (const uint32_t *)((char *)ctx->hb_sc.p + sc_off);
            sc_off += align_up(m.n * fr_bytes, 256);
            HIP_TRY(ctx, hipMemcpyAsync((void *)it[j].scalars, m.scalars, m.n * fr_bytes, hipMemcpyHostToDevice, st));
        } else if (m.index) {
            it[j].index = (const uint32_t *)((char *)ctx->hb_idx.p + idx_off);
            idx_off += align_up(m.n * 4, 256);
            HIP_TRY(ctx, hipMemcpyAsync((void *)it[j].index, m.index, m.n * 4, hipMemcpyHostToDevice, st));
        } else {
            it[j].offset = m.shared_offset;
        }
        if (!it[j].bases) {
            uint32_t *aff = (uint32_t *)((char *)ctx->hb_aff.p + aff_off);
            aff_off += align_up(m.n * aff_bytes, 256);
            HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_src.p, m.bases, m.n * stride, hipMemcpyHostToDevice, st));
            vt->import_bases(st, (const uint32_t *)ctx->hb_src.p, stride / 4, base_form == AMDMSM_FORM_SPECIAL, m.n, aff);
            HIP_TRY(ctx, hipGetLastError());
            it[j].bases = aff;
        }
    }
    amdmsm_opts o = opts_or_default(opts);
    o.stream = st;
    rc = run_batch_items(ctx, vt, k, it, (const uint32_t *)ctx->hb_sc.p, shared_n, flags, &o);
    if (rc) {
        (void)hipDeviceSynchronize();
        return rc;
    }
    // results and flags back after one synchronisation; the outputs are written only when the whole batch is good
    std::vector<char> h_out((size_t)k * xyz_bytes);
    uint32_t h_flags[MAX_BATCH] = {};
    HIP_TRY(ctx, hipMemcpyAsync(h_out.data(), ctx->hb_out.p, (size_t)k * xyz_bytes, hipMemcpyDeviceToHost, st));
    if (flags) HIP_TRY(ctx, hipMemcpyAsync(h_flags, flags, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    rc = check_batch_flags(ctx, k, h_flags);
    if (rc) return rc;
    for (int j = 0; j < k; ++j) memcpy(items[j].out_xyz, h_out.data() + (size_t)j * xyz_bytes, xyz_bytes);
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

// k multi_exp calls of one group and length as ONE batch (amdmsm_msm_device_batch over host vectors): a batch of items
// that all bring their own n scalars.
int amdmsm_multi_exp_batch(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *bases_xyz,
                           size_t base_stride_bytes, int base_form, const void *const *scalars, size_t n,
                           void *const *out_xyz, const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (k < 1 || k > MAX_BATCH || !bases_xyz || !scalars || !out_xyz) return fail(ctx, AMDMSM_ERR_BAD_ARG, "batch of 1 .. 8 MSMs");
    size_t stride = base_stride_bytes;
    for (int j = 0; j < k; ++j) {
        const int rcj = check_host_args(ctx, vt, bases_xyz[j], stride, scalars[j], n, out_xyz[j]);
        if (rcj) return rcj;
    }
    if (k == 1 || n == 0 || n > max_range_points() || (size_t)k * n >= ((size_t)1 << 30)) {
        for (int j = 0; j < k; ++j) {
            const int rcj = host_multi_exp(ctx, vt, bases_xyz[j], stride, base_form, scalars[j], n, out_xyz[j], opts, nullptr);
            if (rcj) return rcj;
        }
        return AMDMSM_OK;
    }
    amdmsm_batch_item items[MAX_BATCH];
    for (int j = 0; j < k; ++j) {
        items[j] = AMDMSM_BATCH_ITEM_INIT;
        items[j].bases = bases_xyz[j];
        items[j].n = n;
        items[j].scalars = scalars[j];
        items[j].out_xyz = out_xyz[j];
    }
    return host_batch_items(ctx, vt, k, items, stride, base_form, nullptr, 0, opts);
}

// k multi_exp calls of one group, each of its own length, as one batch (amdmsm_msm_device_batch_items over host vectors).
int amdmsm_multi_exp_batch_items(amdmsm_ctx *ctx, int curve, int group, int k, const amdmsm_batch_item *items,
                                 size_t base_stride_bytes, int base_form, const void *shared_scalars, size_t shared_n,
                                 const amdmsm_opts *opts) {
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const int rc = check_batch_items(ctx, k, items, shared_scalars, shared_n, true);
    if (rc) return rc;
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    const size_t stride = base_stride_bytes ? base_stride_bytes : xyz_bytes;
    if (stride % rec_align(vt) || stride < xyz_bytes) return fail(ctx, AMDMSM_ERR_BAD_ARG, "base stride");
    if (opts && opts->window_bits > 22) return fail(ctx, AMDMSM_ERR_BAD_ARG, "window_bits > 22 is not available for a batch");
    return host_batch_items(ctx, vt, k, items, stride, base_form, shared_scalars, shared_n, opts);
}

int amdmsm_register_bases(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                          int base_form, size_t n, uint64_t *handle) {
    GET_VT(ctx, curve, group);
    if (!bases_xyz || !n) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null / empty base vector");
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    if (base_stride_bytes == 0) base_stride_bytes = xyz_bytes;
    if (base_stride_bytes % rec_align(vt) || base_stride_bytes < xyz_bytes) return fail(ctx, AMDMSM_ERR_BAD_ARG, "base stride");
    // a re-registration of the same range replaces the old copy
    for (size_t i = ctx->bases.size(); i-- > 0;) {
        const base_entry &e = ctx->bases[i];
        if (e.host == (const char *)bases_xyz && e.curve == curve && e.group == group) drop_entry(ctx, i);
    }
    return register_bases_impl(ctx, vt, bases_xyz, base_stride_bytes, base_form, n, false, handle);
}

int amdmsm_unregister_bases(amdmsm_ctx *ctx, uint64_t handle) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    dev_guard g(ctx->device);
    for (size_t i = 0; i < ctx->bases.size(); ++i) {
        if (ctx->bases[i].id == handle) {
            HIP_TRY(ctx, hipDeviceSynchronize());
            drop_entry(ctx, i);
            return AMDMSM_OK;
        }
    }
    return fail(ctx, AMDMSM_ERR_BAD_ARG, "unknown base handle");
}

int amdmsm_invalidate_bases(amdmsm_ctx *ctx, const void *host_ptr, size_t bytes) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    dev_guard g(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    const char *lo = (const char *)host_ptr, *hi = lo + bytes;
    for (size_t i = ctx->bases.size(); i-- > 0;) {
        const base_entry &e = ctx->bases[i];
        if (!host_ptr || (lo < e.host + e.n * e.stride && hi > e.host)) drop_entry(ctx, i);
    }
    return AMDMSM_OK;
}

// multi_exp across several devices of one node (multiexp.tcc:655-687 with chunk = device):
// context k takes the contiguous range [k*one, (k+1)*one) (the last one the remainder), every
// range runs the whole single-GPU pipeline on its own device from its own host thread, the
// partial points are brought to the first device (hipMemcpyPeerAsync over xGMI) and summed there.
int amdmsm_multi_exp_filter_one_zero_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group, const void *bases_xyz,
                                           size_t base_stride_bytes, int base_form, const void *scalars, size_t n,
                                           void *out_xyz, const amdmsm_opts *opts, size_t stats[3]) {
    if (!ctxs || ndev < 1 || ndev > 64) return AMDMSM_ERR_BAD_ARG;
    for (int k = 0; k < ndev; ++k) {
        if (!ctxs[k]) return AMDMSM_ERR_BAD_ARG;
        for (int j = 0; j < k; ++j) {
            if (ctxs[j] == ctxs[k]) return fail(ctxs[0], AMDMSM_ERR_BAD_ARG, "the same context twice");
        }
    }
    amdmsm_ctx *c0 = ctxs[0];
    CHECK_OPTS(c0, opts);
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return fail(c0, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group");
    if (ndev == 1 || n < (size_t)ndev) {
        if (stats) return amdmsm_multi_exp_filter_one_zero(c0, curve, group, bases_xyz, base_stride_bytes, base_form, scalars,
                                                           n, out_xyz, opts, stats);
        return amdmsm_multi_exp(c0, curve, group, bases_xyz, base_stride_bytes, base_form, scalars, n, out_xyz, opts);
    }
    // lock order = argument order; every caller passing the same list is deadlock-free
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    for (int k = 0; k < ndev; ++k) locks.emplace_back(ctxs[k]->mu);
    size_t stride = base_stride_bytes;
    int rc = check_host_args(c0, vt, bases_xyz, stride, scalars, n, out_xyz);
    if (rc) return rc;
    const size_t xyz_bytes = (size_t)vt->el_words * 12, fr_bytes = (size_t)vt->fr_words * 4;
    const size_t one = n / (size_t)ndev;
    amdmsm_opts o = opts_or_default(opts);
    const int final_form = o.out_form;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    std::vector<int> rcs((size_t)ndev, AMDMSM_OK);
    auto work = [&](int k) {
        amdmsm_ctx *ctx = ctxs[k];
        dev_guard g(ctx->device);
        const size_t lo = (size_t)k * one, cnt = (k == ndev - 1) ? n - lo : one;
        // every device classifies the scalars of its own range (multiexp.tcc:713-733); the counts are added up below
        int r = host_msm_ranges(ctx, vt, (const char *)bases_xyz + lo * stride, stride, base_form,
                                (const char *)scalars + lo * fr_bytes, cnt, &o, stats != nullptr);
        if (r == AMDMSM_OK && hipEventRecord(ctx->host_done, ctx->stream) != hipSuccess) r = AMDMSM_ERR_HIP;
        rcs[(size_t)k] = r;
    };
    std::vector<std::thread> threads;
    for (int k = 1; k < ndev; ++k) threads.emplace_back(work, k);
    work(0);
    for (auto &t : threads) t.join();
    int failed = -1;
    for (int k = 0; k < ndev; ++k) {
        if (rcs[(size_t)k] && failed < 0) failed = k;
    }
    dev_guard g0(c0->device);
    if (failed >= 0) {
        for (int k = 0; k < ndev; ++k) {
            dev_guard g(ctxs[k]->device);
            (void)hipDeviceSynchronize();
        }
        // amdmsm_last_error is asked of the first context: carry the failing range's message over
        return fail(c0, rcs[(size_t)failed], "range " + std::to_string(failed) + ": " + ctxs[failed]->err);
    }
    rc = ensure_partials(c0);
    if (rc) return rc;
    hipStream_t st = c0->stream;
    for (int k = 0; k < ndev; ++k) {
        HIP_TRY(c0, hipStreamWaitEvent(st, ctxs[k]->host_done, 0));
        HIP_TRY(c0, copy_partial(st, (char *)c0->chunk_partials + (size_t)k * xyz_bytes, c0->device, ctxs[k]->hb_out.p,
                                 ctxs[k]->device, xyz_bytes));
    }
    // (device 0's own partial has been copied out of hb_out by the loop above, in stream order)
    vt->sum_points(st, (const uint32_t *)c0->chunk_partials, ndev, final_form, (uint32_t *)c0->hb_out.p);
    HIP_TRY(c0, hipGetLastError());
    HIP_TRY(c0, hipMemcpyAsync(out_xyz, c0->hb_out.p, xyz_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c0, hipStreamSynchronize(st));
    size_t zeros = 0, ones = 0;
    for (int k = 0; k < ndev; ++k) {
        dev_guard g(ctxs[k]->device);
        HIP_TRY(c0, hipStreamSynchronize(ctxs[k]->copy_stream));
        HIP_TRY(c0, hipStreamSynchronize(ctxs[k]->stream));
        if (stats) {
            uint32_t hs[4] = {};
            HIP_TRY(c0, hipMemcpy(hs, ctxs[k]->hb_stats.p, 16, hipMemcpyDeviceToHost));
            zeros += hs[0];
            ones += hs[1];
        }
    }
    if (stats) {
        stats[0] = zeros;
        stats[1] = ones;
        stats[2] = n - zeros - ones;
    }
    return AMDMSM_OK;
}

int amdmsm_multi_exp_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group, const void *bases_xyz,
                           size_t base_stride_bytes, int base_form, const void *scalars, size_t n, void *out_xyz,
                           const amdmsm_opts *opts) {
    return amdmsm_multi_exp_filter_one_zero_multi(ctxs, ndev, curve, group, bases_xyz, base_stride_bytes, base_form, scalars, n,
                                                  out_xyz, opts, nullptr);
}

// Device-resident counterpart: context k holds its own range (compact affine bases + scalars)
// in its own HBM; partial k is reduced on device k and the partials are summed on device 0.
int amdmsm_msm_device_multi(amdmsm_ctx *const *ctxs, int ndev, int curve, int group, const void *const *d_bases_affine,
                            const void *const *d_scalars, const size_t *counts, void *d_out_xyz_dev0,
                            const amdmsm_opts *opts) {
    if (!ctxs || ndev < 1 || ndev > 64 || !d_bases_affine || !d_scalars || !counts || !d_out_xyz_dev0) return AMDMSM_ERR_BAD_ARG;
    for (int k = 0; k < ndev; ++k) {
        if (!ctxs[k]) return AMDMSM_ERR_BAD_ARG;
        for (int j = 0; j < k; ++j) {
            if (ctxs[j] == ctxs[k]) return fail(ctxs[0], AMDMSM_ERR_BAD_ARG, "the same context twice");
        }
    }
    amdmsm_ctx *c0 = ctxs[0];
    CHECK_OPTS(c0, opts);
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return fail(c0, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group");
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    for (int k = 0; k < ndev; ++k) locks.emplace_back(ctxs[k]->mu);
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    amdmsm_opts o = opts_or_default(opts);
    const int final_form = o.out_form;
    hipStream_t user_stream = (hipStream_t)o.stream;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    o.stream = nullptr;
    // The ranges run on the contexts' own streams.  Inputs the caller produced on opts->stream are
    // ordered before them: every context stream waits for an event recorded on that stream now.
    if (user_stream) {
        dev_guard g(c0->device);
        HIP_TRY(c0, hipEventRecord(c0->bases_ready, user_stream));
    }
    // kernels are asynchronous: one host thread enqueues all devices
    int rc = AMDMSM_OK, failed = -1;
    for (int k = 0; k < ndev && rc == AMDMSM_OK; ++k) {
        amdmsm_ctx *ctx = ctxs[k];
        dev_guard g(ctx->device);
        failed = k;
        rc = ensure_buf(ctx, ctx->hb_out, xyz_bytes);
        if (rc) break;
        if (counts[k] && (!d_bases_affine[k] || !d_scalars[k])) {
            rc = fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
            break;
        }
        if (user_stream && hipStreamWaitEvent(ctx->stream, c0->bases_ready, 0) != hipSuccess) {
            rc = fail(ctx, AMDMSM_ERR_HIP, "hipStreamWaitEvent");
            break;
        }
        rc = msm_device_ranges(ctx, vt, (const uint32_t *)d_bases_affine[k], (const uint32_t *)d_scalars[k], counts[k],
                               (uint32_t *)ctx->hb_out.p, &o);
        if (rc) break;
        if (hipEventRecord(ctx->host_done, ctx->stream) != hipSuccess) rc = fail(ctx, AMDMSM_ERR_HIP, "hipEventRecord");
    }
    if (rc) {
        // nothing of this call may still be in flight when the caller reads the error
        for (int k = 0; k < ndev; ++k) {
            dev_guard g(ctxs[k]->device);
            (void)hipDeviceSynchronize();
        }
        return fail(c0, rc, "range " + std::to_string(failed) + ": " + ctxs[failed]->err);
    }
    dev_guard g0(c0->device);
    rc = ensure_partials(c0);
    if (rc) return rc;
    hipStream_t st = user_stream ? user_stream : c0->stream;
    for (int k = 0; k < ndev; ++k) {
        HIP_TRY(c0, hipStreamWaitEvent(st, ctxs[k]->host_done, 0));
        HIP_TRY(c0, copy_partial(st, (char *)c0->chunk_partials + (size_t)k * xyz_bytes, c0->device, ctxs[k]->hb_out.p,
                                 ctxs[k]->device, xyz_bytes));
    }
    vt->sum_points(st, (const uint32_t *)c0->chunk_partials, ndev, final_form, (uint32_t *)d_out_xyz_dev0);
    HIP_TRY(c0, hipGetLastError());
    HIP_TRY(c0, hipStreamSynchronize(st));   // the partials buffer is shared by the context
    return AMDMSM_OK;
}

}   // extern "C"

namespace {
// multi_exp_stream (multiexp_stream.hpp:25-33, multiexp_stream.tcc:164-191): the bases arrive
// through a reader in libff's on-disk format and never have to be resident at once.  Chunks of
// `chunk_points` records are read into pinned staging buffers, copied and decoded on the
// device, and reduced to one partial point each on alternating streams / workspace slots, so
// reading chunk k+1 overlaps the MSM of chunk k; the partials are summed at the end
// (multiexp.tcc:681-687).
// recs = records per scalar in the stream: 1 for multi_exp_stream; for the precompute variant the
// num_digits multiples [2^(jc)]P of each base, consumed with window size precompute_c
// (element_buffers_from_stream_producer, multiexp_stream.tcc:33-49).
// compressed: the records hold X and two flag bits only (compression_on, curve_serialization.tcc:
// 103-166); Y is recovered on the device by a square root.
int stream_impl(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read, void *read_ctx, const void *scalars,
                size_t n, size_t chunk_points, void *out_xyz, const amdmsm_opts *opts, size_t recs,
                size_t precompute_c, bool compressed = false) {
    if (!ctx || !read || !out_xyz || (n && !scalars)) return AMDMSM_ERR_BAD_ARG;
    CHECK_OPTS(ctx, opts);
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group");
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8 * recs;
    const size_t rec_bytes = compressed ? aff_bytes / 2 : aff_bytes;   // bytes in the stream per scalar
    const size_t fr_bytes = (size_t)vt->fr_words * 4;
    if (chunk_points == 0) chunk_points = std::max<size_t>(((size_t)1 << 20) / recs, 1024);
    if (chunk_points > n && n) chunk_points = n;
    const size_t nchunks = n ? (n + chunk_points - 1) / chunk_points : 0;
    constexpr int NB = stream_state::NB;
    // the call owns the context from here on: it changes the pipeline depth and the slot rotation
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    const int old_depth = ctx->depth;
    dev_guard guard(ctx->device);
    stream_state &ss = ctx->ss;
    // Staging lives in the context and only grows: pinned host buffers, device buffers and the two streams are
    // set up by the first call (2 x 64 MiB of pinned memory cost ~40 ms to allocate), later calls reuse them.
    auto finish = [&](int rc_) {
        (void)hipDeviceSynchronize();
        (void)amdmsm_set_pipeline_depth(ctx, old_depth);
        return rc_;
    };
#define TRY_S(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return finish(fail(ctx, AMDMSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); \
    } while (0)
    int rc = amdmsm_set_pipeline_depth(ctx, NB);
    if (rc) return rc;
    rc = ensure_buf(ctx, ss.partials, (nchunks + 1) * xyz_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ss.status, 16);
    for (int b = 0; b < NB && nchunks && rc == AMDMSM_OK; ++b) {
        if (ss.h_bytes[b] < chunk_points * aff_bytes) {
            (void)hipDeviceSynchronize();
            if (ss.h_stage[b]) (void)hipHostFree(ss.h_stage[b]);
            ss.h_stage[b] = nullptr;
            ss.h_bytes[b] = 0;
            TRY_S(hipHostMalloc(&ss.h_stage[b], chunk_points * aff_bytes, hipHostMallocDefault));
            ss.h_bytes[b] = chunk_points * aff_bytes;
        }
        rc = ensure_buf(ctx, ss.d_raw[b], chunk_points * aff_bytes);
        if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ss.d_aff[b], chunk_points * aff_bytes);
        if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ss.d_sc[b], chunk_points * fr_bytes);
        if (rc == AMDMSM_OK && !ss.streams[b]) TRY_S(hipStreamCreateWithFlags(&ss.streams[b], hipStreamNonBlocking));
    }
    if (rc) return finish(rc);
    void *d_partials = ss.partials.p, *d_status = ss.status.p;
    TRY_S(hipMemsetAsync(d_status, 0, 16, ctx->stream));
    TRY_S(hipStreamSynchronize(ctx->stream));
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    if (opts) o = *opts;
    const int final_form = opts ? opts->out_form : AMDMSM_OUT_LIBFF;
    o.out_form = AMDMSM_OUT_JACOBIAN;
    for (size_t k = 0; k < nchunks; ++k) {
        const int b = (int)(k % NB);
        const size_t lo = k * chunk_points, cnt = std::min(chunk_points, n - lo);
        TRY_S(hipStreamSynchronize(ss.streams[b]));   // staging buffer b is free again
        const size_t want = cnt * rec_bytes;
        size_t got = 0;
        while (got < want) {
            const size_t r = read(read_ctx, (char *)ss.h_stage[b] + got, want - got);
            if (r == 0) break;
            got += r;
        }
        if (got != want) return finish(fail(ctx, AMDMSM_ERR_BAD_ARG, "base-element stream ended early"));
        TRY_S(hipMemcpyAsync(ss.d_raw[b].p, ss.h_stage[b], want, hipMemcpyHostToDevice, ss.streams[b]));
        TRY_S(hipMemcpyAsync(ss.d_sc[b].p, (const char *)scalars + lo * fr_bytes, cnt * fr_bytes, hipMemcpyHostToDevice,
                             ss.streams[b]));
        if (compressed)
            vt->disk_decode_compressed(ss.streams[b], (const uint32_t *)ss.d_raw[b].p, cnt * recs, (uint32_t *)ss.d_aff[b].p,
                                       (uint32_t *)d_status);
        else
            vt->disk_decode(ss.streams[b], (const uint32_t *)ss.d_raw[b].p, cnt * recs, (uint32_t *)ss.d_aff[b].p);
        o.stream = ss.streams[b];
        if (precompute_c)
            rc = amdmsm_msm_precomputed_device(ctx, curve, group, ss.d_aff[b].p, ss.d_sc[b].p, cnt, precompute_c, recs,
                                               (char *)d_partials + k * xyz_bytes, &o);
        else
            rc = amdmsm_msm_device(ctx, curve, group, ss.d_aff[b].p, ss.d_sc[b].p, cnt, (char *)d_partials + k * xyz_bytes, &o);
        if (rc) return finish(rc);
    }
    TRY_S(hipDeviceSynchronize());
    vt->sum_points(ctx->stream, (const uint32_t *)d_partials, (int)nchunks, final_form,
                   (uint32_t *)((char *)d_partials + nchunks * xyz_bytes));
    unsigned status = 0;
    TRY_S(hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    TRY_S(hipStreamSynchronize(ctx->stream));
    // some X is not the abscissa of a curve point: no result (the reference's sqrt would not return)
    if (status) return finish(fail(ctx, AMDMSM_ERR_BAD_ARG, "compressed base element is not on the curve"));
    TRY_S(hipMemcpyAsync(out_xyz, (char *)d_partials + nchunks * xyz_bytes, xyz_bytes, hipMemcpyDeviceToHost, ctx->stream));
    TRY_S(hipStreamSynchronize(ctx->stream));
    return finish(AMDMSM_OK);
#undef TRY_S
}

// file reader of the *_file entries: the chunk is read by several threads at once, each with pread on its own
// slice (one thread copies from the page cache at ~3.5 GB/s, less than the PCIe link takes)
struct file_src {
    int fd = -1;
    size_t pos = 0;
};
size_t file_reader(void *ctxp, void *dst, size_t bytes) {
    file_src &f = *(file_src *)ctxp;
    constexpr size_t SLICE = (size_t)8 << 20;
    static const unsigned max_threads = [] {
        const char *e = getenv("AMDMSM_READ_THREADS");
        const unsigned hw = std::thread::hardware_concurrency();
        const unsigned def = std::min(8u, std::max(1u, hw / 2));
        return e && atoi(e) > 0 ? (unsigned)atoi(e) : def;
    }();
    const size_t slices = (bytes + SLICE - 1) / SLICE;
    const unsigned nt = (unsigned)std::min<size_t>(max_threads, slices);
    std::vector<size_t> got((size_t)std::max(nt, 1u), 0);
    auto work = [&](unsigned t) {
        for (size_t sidx = t; sidx < slices; sidx += nt) {
            size_t off = sidx * SLICE;
            const size_t end = std::min(bytes, off + SLICE);
            while (off < end) {
                const ssize_t r = pread(f.fd, (char *)dst + off, end - off, (off_t)(f.pos + off));
                if (r <= 0) return;
                off += (size_t)r;
                got[t] += (size_t)r;
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    size_t total = 0;
    for (size_t g : got) total += g;
    if (total != bytes) {
        // short file: report the contiguous prefix only (the caller treats a short read as the end of the stream)
        struct stat st;
        const size_t size = fstat(f.fd, &st) == 0 ? (size_t)st.st_size : 0;
        total = size > f.pos ? std::min(bytes, size - f.pos) : 0;
        if (total == bytes) total = 0;
    }
    f.pos += total;
    return total;
}

int stream_file_impl(amdmsm_ctx *ctx, int curve, int group, const char *path, size_t offset_bytes, const void *scalars,
                     size_t n, size_t chunk_points, void *out_xyz, const amdmsm_opts *opts, size_t recs,
                     size_t precompute_c, bool compressed = false) {
    if (!ctx || !path) return AMDMSM_ERR_BAD_ARG;
    file_src f;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string("cannot open ") + path);
    f.pos = offset_bytes;
    const int rc = stream_impl(ctx, curve, group, file_reader, &f, scalars, n, chunk_points, out_xyz, opts, recs,
                               precompute_c, compressed);
    close(f.fd);
    return rc;
}

// A device vector of point records or of on-disk records: the kernels move the records 16 bytes at a time, 8 for the
// 10-word fields (rec_align); two vectors of one call may not share a byte
int dev_check_aligned(amdmsm_ctx *ctx, const char *what, const void *p, size_t align) {
    if ((uintptr_t)p & (align - 1)) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(what) + ": not aligned to " + std::to_string(align) + " bytes");
    return AMDMSM_OK;
}
bool dev_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// what the three encoding entries refuse before they look at the context: a group the library does not carry, and
// compressed records of an a != 0 curve (the decoder's rule and message)
int encode_refuse(amdmsm_ctx *ctx, int curve, int group, int compressed) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group");
    if (compressed && vt->coeff_a_nonzero) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "compressed records: a != 0 curve");
    return AMDMSM_OK;
}
// ... and what they ask of the resident source vector (the caller has the context's lock)
int encode_check_source(amdmsm_ctx *ctx, const group_vtable *vt, const void *d_points_affine, size_t n) {
    if (n && !d_points_affine) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    return n ? dev_check_aligned(ctx, "d_points_affine", d_points_affine, rec_align(vt)) : AMDMSM_OK;
}
void encode_launch(const group_vtable *vt, hipStream_t st, const void *d_src, size_t n, bool compressed, void *d_dst) {
    if (compressed) vt->disk_encode_compressed(st, (const uint32_t *)d_src, n, (uint32_t *)d_dst);
    else vt->disk_encode(st, (const uint32_t *)d_src, n, (uint32_t *)d_dst);
}

// The writer twin of stream_impl: n compact affine records in HBM leave as libff's on-disk records through `write`,
// write_plan.h's chunks one after the other.  Chunk k is encoded on the device and copied into pinned staging buffer
// k % 2 on stream k % 2 (the staging buffers, device buffers and streams of the readers); while that runs the host
// hands chunk k - 1 to `write`, one call per chunk, in order.  The source has to be complete on the context's stream.
// A callback that takes fewer bytes than offered ends the call, as a reader that delivers too few ends stream_impl.
int write_impl(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n, bool compressed,
               amdmsm_write_fn write, void *write_ctx, size_t chunk_points) {
    int rc = encode_refuse(ctx, curve, group, compressed);
    if (rc) return rc;
    if (!ctx || !write) return AMDMSM_ERR_BAD_ARG;
    const group_vtable *vt = find_vt(curve, group);
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    dev_guard guard(ctx->device);
    rc = encode_check_source(ctx, vt, d_points_affine, n);
    if (rc) return rc;
    const size_t aff_bytes = (size_t)vt->el_words * 8, rec_bytes = compressed ? aff_bytes / 2 : aff_bytes;
    const write_plan plan = write_plan_of(n, chunk_points);
    if (!plan.nchunks) return AMDMSM_OK;
    constexpr int NB = stream_state::NB;
    static_assert(NB == WRITE_BUFFERS, "the plan's buffers are the readers' staging buffers");
    stream_state &ss = ctx->ss;
    auto finish = [&](int rc_) {
        for (int b = 0; b < NB; ++b) {
            if (ss.streams[b]) (void)hipStreamSynchronize(ss.streams[b]);   // nothing of this call may still write the staging
        }
        return rc_;
    };
#define TRY_W(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return finish(fail(ctx, AMDMSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); \
    } while (0)
    const size_t stage_bytes = plan.chunk_points * rec_bytes;
    for (int b = 0; b < NB && (size_t)b < plan.nchunks; ++b) {
        if (ss.h_bytes[b] < stage_bytes) {
            (void)hipDeviceSynchronize();
            if (ss.h_stage[b]) (void)hipHostFree(ss.h_stage[b]);
            ss.h_stage[b] = nullptr;
            ss.h_bytes[b] = 0;
            TRY_W(hipHostMalloc(&ss.h_stage[b], stage_bytes, hipHostMallocDefault));
            ss.h_bytes[b] = stage_bytes;
        }
        rc = ensure_buf(ctx, ss.d_raw[b], stage_bytes);
        if (rc) return finish(rc);
        if (!ss.streams[b]) TRY_W(hipStreamCreateWithFlags(&ss.streams[b], hipStreamNonBlocking));
    }
    // the two streams do not wait for the context's stream by themselves
    TRY_W(hipEventRecord(ctx->bases_ready, ctx->stream));
    for (int b = 0; b < NB && (size_t)b < plan.nchunks; ++b) TRY_W(hipStreamWaitEvent(ss.streams[b], ctx->bases_ready, 0));
    auto hand_over = [&](size_t k) {   // chunk k, whose copy is enqueued on its stream, to the callback
        const write_chunk c = write_plan_chunk(plan, k);
        TRY_W(hipStreamSynchronize(ss.streams[c.buffer]));
        const size_t bytes = c.count * rec_bytes;
        if (write(write_ctx, ss.h_stage[c.buffer], bytes) != bytes) return finish(fail(ctx, AMDMSM_ERR_BAD_ARG, "record stream ended early"));
        return (int)AMDMSM_OK;
    };
    for (size_t k = 0; k < plan.nchunks; ++k) {
        const write_chunk c = write_plan_chunk(plan, k);   // buffer c.buffer is free: chunk k - 2 has been handed over
        hipStream_t st = ss.streams[c.buffer];
        encode_launch(vt, st, (const char *)d_points_affine + c.first * aff_bytes, c.count, compressed, ss.d_raw[c.buffer].p);
        TRY_W(hipGetLastError());
        TRY_W(hipMemcpyAsync(ss.h_stage[c.buffer], ss.d_raw[c.buffer].p, c.count * rec_bytes, hipMemcpyDeviceToHost, st));
        if (k) {
            rc = hand_over(k - 1);
            if (rc) return rc;
        }
    }
    rc = hand_over(plan.nchunks - 1);
    if (rc) return rc;
    return finish(AMDMSM_OK);
#undef TRY_W
}

// the callback of amdmsm_write_points_file: pwrite at the file's running offset, whatever number of calls that takes
struct file_dst {
    int fd = -1;
    size_t pos = 0;
    bool failed = false;
};
size_t file_writer(void *ctxp, const void *src, size_t bytes) {
    file_dst &f = *(file_dst *)ctxp;
    size_t done = 0;
    while (done < bytes) {
        const ssize_t w = pwrite(f.fd, (const char *)src + done, bytes - done, (off_t)(f.pos + done));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            f.failed = true;
            break;
        }
        done += (size_t)w;
    }
    f.pos += done;
    return done;
}
}  // namespace

extern "C" {

int amdmsm_multi_exp_stream(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read, void *read_ctx,
                            const void *scalars, size_t n, size_t chunk_points, void *out_xyz,
                            const amdmsm_opts *opts) {
    return stream_impl(ctx, curve, group, read, read_ctx, scalars, n, chunk_points, out_xyz, opts, 1, 0);
}

int amdmsm_multi_exp_stream_file(amdmsm_ctx *ctx, int curve, int group, const char *path, size_t offset_bytes,
                                 const void *scalars, size_t n, size_t chunk_points, void *out_xyz,
                                 const amdmsm_opts *opts) {
    return stream_file_impl(ctx, curve, group, path, offset_bytes, scalars, n, chunk_points, out_xyz, opts, 1, 0);
}

// multi_exp_stream<form_montgomery, compression_on, G, Fr> (multiexp_stream.hpp:25-27 with
// Comp = compression_on; records of curve_serialization.tcc:103-133)
int amdmsm_multi_exp_stream_compressed(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read, void *read_ctx,
                                       const void *scalars, size_t n, size_t chunk_points, void *out_xyz,
                                       const amdmsm_opts *opts) {
    const group_vtable *vt = find_vt(curve, group);
    if (vt && vt->coeff_a_nonzero) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "compressed records: a != 0 curve");
    return stream_impl(ctx, curve, group, read, read_ctx, scalars, n, chunk_points, out_xyz, opts, 1, 0, true);
}

int amdmsm_multi_exp_stream_compressed_file(amdmsm_ctx *ctx, int curve, int group, const char *path, size_t offset_bytes,
                                            const void *scalars, size_t n, size_t chunk_points, void *out_xyz,
                                            const amdmsm_opts *opts) {
    const group_vtable *vt = find_vt(curve, group);
    if (vt && vt->coeff_a_nonzero) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "compressed records: a != 0 curve");
    return stream_file_impl(ctx, curve, group, path, offset_bytes, scalars, n, chunk_points, out_xyz, opts, 1, 0, true);
}

// group_read<encoding_binary, form_montgomery, Comp> over an array of records already in HBM
// (curve_serialization.tcc:78-101 / 134-166): n compact affine points out.
int amdmsm_disk_decode_device(amdmsm_ctx *ctx, int curve, int group, const void *d_records, size_t n, int compressed,
                              void *d_dst_affine, unsigned *status) {
    GET_VT(ctx, curve, group);
    if (compressed && vt->coeff_a_nonzero) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "compressed records: a != 0 curve");
    if (n && (!d_records || !d_dst_affine)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    hipStream_t st = ctx->stream;
    unsigned hs = 0;
    if (compressed) {
        int rc = ensure_buf(ctx, ctx->hb_stats, 16);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->hb_stats.p, 0, 16, st));
        vt->disk_decode_compressed(st, (const uint32_t *)d_records, n, (uint32_t *)d_dst_affine, (uint32_t *)ctx->hb_stats.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&hs, ctx->hb_stats.p, 4, hipMemcpyDeviceToHost, st));
    } else {
        vt->disk_decode(st, (const uint32_t *)d_records, n, (uint32_t *)d_dst_affine);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (status) *status = hs;
    return AMDMSM_OK;
}

// group_write<encoding_binary, form_montgomery, Comp> over n compact affine points in HBM (curve_serialization.tcc:
// 78-133), the inverse of amdmsm_disk_decode_device: n records out, enqueued on `stream` and not waited for.
int amdmsm_disk_encode_device(amdmsm_ctx *ctx, int curve, int group, const void *d_src_affine, size_t n, int compressed,
                              void *d_records, void *stream) {
    int rc = encode_refuse(ctx, curve, group, compressed);
    if (rc) return rc;
    GET_VT(ctx, curve, group);
    rc = encode_check_source(ctx, vt, d_src_affine, n);
    if (rc || !n) return rc;
    if (!d_records) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    rc = dev_check_aligned(ctx, "d_records", d_records, rec_align(vt));
    if (rc) return rc;
    const size_t aff_bytes = (size_t)vt->el_words * 8;
    if (dev_ranges_overlap(d_src_affine, n * aff_bytes, d_records, n * (compressed ? aff_bytes / 2 : aff_bytes)))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "d_records overlaps d_src_affine");
    encode_launch(vt, stream ? (hipStream_t)stream : ctx->stream, d_src_affine, n, compressed != 0, d_records);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_plan_write_points(size_t n, size_t chunk_points, size_t k, size_t out[4]) {
    if (!out) return AMDMSM_ERR_BAD_ARG;
    const write_plan p = write_plan_of(n, chunk_points);
    out[0] = p.nchunks;
    out[1] = out[2] = out[3] = 0;
    if (k >= p.nchunks) return AMDMSM_OK;
    const write_chunk c = write_plan_chunk(p, k);
    out[1] = c.first;
    out[2] = c.count;
    out[3] = (size_t)c.buffer;
    return AMDMSM_OK;
}

int amdmsm_write_points_stream(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n, int compressed,
                               amdmsm_write_fn write, void *write_ctx, size_t chunk_points) {
    return write_impl(ctx, curve, group, d_points_affine, n, compressed != 0, write, write_ctx, chunk_points);
}

// the file is opened without truncation and created where absent; the bytes in front of offset_bytes and behind the
// records stay as they are (the readers' offset_bytes, mirrored)
int amdmsm_write_points_file(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n, int compressed,
                             const char *path, size_t offset_bytes, size_t chunk_points) {
    int rc = encode_refuse(ctx, curve, group, compressed);
    if (rc) return rc;
    if (!ctx || !path) return AMDMSM_ERR_BAD_ARG;
    {   // a refused call creates no file
        std::lock_guard<std::recursive_mutex> lock(ctx->mu);
        rc = encode_check_source(ctx, find_vt(curve, group), d_points_affine, n);
        if (rc) return rc;
    }
    file_dst f;
    f.fd = open(path, O_WRONLY | O_CREAT, 0644);
    if (f.fd < 0) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string("cannot open ") + path);
    f.pos = offset_bytes;
    rc = write_impl(ctx, curve, group, d_points_affine, n, compressed != 0, file_writer, &f, chunk_points);
    if (close(f.fd) != 0) f.failed = true;
    if (f.failed) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string("cannot write ") + path);
    return rc;
}

// multi_exp_stream_with_precompute (multiexp_stream.hpp:29-42, multiexp_stream.tcc:193-223): the
// stream holds, per base, the num_digits = ceil(Fr::num_bits / c) multiples [2^(jc)]P; every
// (scalar digit, multiple) pair lands in ONE bucket set and no doublings are needed.  Like the
// reference, a carry out of the last digit is dropped (it cannot occur when the top digit has
// spare bits, e.g. the 254-bit alt_bn128 Fr with c = 16).
int amdmsm_multi_exp_stream_with_precompute(amdmsm_ctx *ctx, int curve, int group, amdmsm_read_fn read, void *read_ctx,
                                            const void *scalars, size_t n, size_t precompute_c, size_t chunk_points,
                                            void *out_xyz, const amdmsm_opts *opts) {
    const size_t recs = amdmsm_precompute_num_digits(curve, precompute_c);
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    if (precompute_c < 2 || precompute_c > 22 || !recs) return fail(ctx, AMDMSM_ERR_BAD_ARG, "precompute_c must be 2..22");
    return stream_impl(ctx, curve, group, read, read_ctx, scalars, n, chunk_points, out_xyz, opts, recs, precompute_c);
}

int amdmsm_multi_exp_stream_with_precompute_file(amdmsm_ctx *ctx, int curve, int group, const char *path,
                                                 size_t offset_bytes, const void *scalars, size_t n,
                                                 size_t precompute_c, size_t chunk_points, void *out_xyz,
                                                 const amdmsm_opts *opts) {
    const size_t recs = amdmsm_precompute_num_digits(curve, precompute_c);
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    if (precompute_c < 2 || precompute_c > 22 || !recs) return fail(ctx, AMDMSM_ERR_BAD_ARG, "precompute_c must be 2..22");
    return stream_file_impl(ctx, curve, group, path, offset_bytes, scalars, n, chunk_points, out_xyz, opts, recs,
                            precompute_c);
}

int amdmsm_batch_exp(amdmsm_ctx *ctx, int curve, int group, size_t scalar_size, size_t window, const void *g_xyz,
                     const void *scalars, size_t n, const void *coeff, int scalars_plain, void *out_xyz) {
    GET_VT(ctx, curve, group);
    if (!g_xyz || (n && (!scalars || !out_xyz))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (window < 1 || window > 22 || scalar_size < 1 || scalar_size > (size_t)vt->fr_words * 32) {
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "window / scalar_size");
    }
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8, fr_bytes = (size_t)vt->fr_words * 4;
    const size_t outerc = (scalar_size + window - 1) / window;
    const size_t entries = outerc << window;
    hipStream_t st = ctx->stream;
    // Device buffers are the context's (grow-only), and the affine window table stays in HBM: a key
    // generator calls batch_exp many times with one table (libsnark r1cs_gg_ppzksnark_generator), so a
    // call with the same (group, scalar_size, window, g) as the last one skips get_window_table's work.
    fb_state &fb = ctx->fb;
    const bool same_table = fb.valid && fb.curve == curve && fb.group == group && fb.scalar_size == scalar_size &&
                            fb.window == window && memcmp(fb.g, g_xyz, xyz_bytes) == 0;
    int rc = ensure_buf(ctx, fb.small, 2 * xyz_bytes + outerc * xyz_bytes + 64);
    if (rc == AMDMSM_OK && !same_table) {
        fb.valid = false;
        rc = ensure_buf(ctx, fb.table, entries * xyz_bytes);
        if (rc == AMDMSM_OK) rc = ensure_buf(ctx, fb.table_aff, entries * aff_bytes);
    }
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_sc, n ? n * fr_bytes : 16);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, fb.out, n ? n * xyz_bytes : 16);
    if (rc) return rc;
    char *d_g = (char *)fb.small.p, *d_cf = d_g + xyz_bytes, *d_go = d_cf + xyz_bytes;
    // a call of amdmsm_batch_exp_device on another stream may still read the table and the coefficient slot
    if (fb.used_valid) HIP_TRY(ctx, hipStreamWaitEvent(st, fb.used, 0));
    ctx->aux_pending = false;
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[0], st));
    if (!same_table) {
        HIP_TRY(ctx, hipMemcpyAsync(d_g, g_xyz, xyz_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(fb.table.p, 0, entries * xyz_bytes, st));   // rows shorter than 2^window: infinity beyond
    }
    if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, scalars, n * fr_bytes, hipMemcpyHostToDevice, st));
    if (coeff) HIP_TRY(ctx, hipMemcpyAsync(d_cf, coeff, fr_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[1], st));
    // table build and exponentiation are separate launches of the same entry: time them apart
    if (!same_table) {
        vt->fixed_base_exp(st, (const uint32_t *)d_g, (int)scalar_size, (int)window, nullptr, 0, 0, nullptr, AMDMSM_OUT_LIBFF,
                           (uint32_t *)d_go, (uint32_t *)fb.table.p, (uint32_t *)fb.table_aff.p, 1, nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[2], st));
    vt->fixed_base_exp(st, (const uint32_t *)d_g, (int)scalar_size, (int)window, (const uint32_t *)ctx->hb_sc.p, n,
                       scalars_plain ? 0 : 1, coeff ? (const uint32_t *)d_cf : nullptr, AMDMSM_OUT_LIBFF, (uint32_t *)d_go,
                       (uint32_t *)fb.table.p, (uint32_t *)fb.table_aff.p, 0, (uint32_t *)fb.out.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[3], st));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(out_xyz, fb.out.p, n * xyz_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[4], st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ctx->aux_ms[i], ctx->aux_ev[i], ctx->aux_ev[i + 1]);
    if (same_table) ctx->aux_ms[1] = 0;   // two adjacent events: nothing was built
    fb.valid = true;
    fb.curve = curve;
    fb.group = group;
    fb.scalar_size = scalar_size;
    fb.window = window;
    memcpy(fb.g, g_xyz, xyz_bytes);
    return AMDMSM_OK;
}

// device times of the last amdmsm_batch_exp of this context: ms[0] inputs host -> device, ms[1] window table
// (0 when the resident table was reused), ms[2] the exponentiations (k_fb_exp), ms[3] results device -> host.
// After amdmsm_batch_exp_device, which returns with its work enqueued: the call is waited for here, ms[0] is the upload
// of g / coeff and ms[3] the normalisation (0 for AMDMSM_OUT_LIBFF).
int amdmsm_get_batch_exp_timings(amdmsm_ctx *ctx, float ms[4]) {
    if (!ctx || !ms) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (ctx->aux_pending) {
        dev_guard guard(ctx->device);
        HIP_TRY(ctx, hipEventSynchronize(ctx->aux_ev[4]));
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ctx->aux_ms[i], ctx->aux_ev[i], ctx->aux_ev[i + 1]);
        if (ctx->aux_reused) ctx->aux_ms[1] = 0;
        if (!ctx->aux_normalised) ctx->aux_ms[3] = 0;
        ctx->aux_pending = false;
    }
    for (int i = 0; i < 4; ++i) ms[i] = ctx->aux_ms[i];
    return AMDMSM_OK;
}

int amdmsm_batch_to_special(amdmsm_ctx *ctx, int curve, int group, void *elems_xyz, size_t stride_bytes, size_t n) {
    GET_VT(ctx, curve, group);
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    if (stride_bytes == 0) stride_bytes = xyz_bytes;
    if (stride_bytes != xyz_bytes) return fail(ctx, AMDMSM_ERR_BAD_ARG, "batch_to_special needs packed records");
    if (!n) return AMDMSM_OK;
    hipStream_t st = ctx->stream;
    void *d_src = nullptr, *d_aff = nullptr;
    HIP_TRY(ctx, hipMalloc(&d_src, n * xyz_bytes));
    if (hipMalloc(&d_aff, n * aff_bytes) != hipSuccess) {
        (void)hipFree(d_src);
        return fail(ctx, AMDMSM_ERR_HIP, "hipMalloc");
    }
    hipError_t e = hipMemcpyAsync(d_src, elems_xyz, n * xyz_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        vt->import_bases(st, (const uint32_t *)d_src, xyz_bytes / 4, 0, n, (uint32_t *)d_aff);
        vt->export_affine(st, (const uint32_t *)d_aff, n, (uint32_t *)d_src);
        e = hipMemcpyAsync(elems_xyz, d_src, n * xyz_bytes, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_src);
    (void)hipFree(d_aff);
    if (e != hipSuccess) return fail(ctx, AMDMSM_ERR_HIP, hipGetErrorString(e));
    return AMDMSM_OK;
}

}  // extern "C"

// ---- element-wise scalar multiplication: out[i] = k_i * P_i ---------------------------------------------------------
namespace {

// What the point-vector entries (this one, fold_vec, group_fft, the segmented MSM) share.
//
// The per-element table (group_vtable::smv_table) is smv_entries compact affine records per element, and its scratch as
// much again, so a vector is worked through in chunks.  chunk_points = 0 picks the chunk from a workspace budget of
// 1 GiB: the largest multiple of 256 elements that fits beside the call's fixed part (at least 256); never more than
// `limit` elements.
constexpr size_t SMV_WS_BUDGET = (size_t)1 << 30;
size_t smv_table_bytes(const group_vtable *vt, size_t cn) { return (size_t)vt->smv_entries * cn * (size_t)vt->el_words * 8; }
size_t vec_chunk_points(size_t bytes_per_element, size_t fixed_bytes, size_t limit, size_t chunk_points) {
    size_t cn = chunk_points;
    if (!cn) {
        cn = (SMV_WS_BUDGET - fixed_bytes) / bytes_per_element / 256 * 256;
        if (cn < 256) cn = 256;
    }
    return cn < limit ? cn : limit;
}

// What the kernels are told of the caller's options: whether the scalars are in Montgomery form, and the form of the
// results.  The kernels write libff records when the caller wants affine ones; vec_finish then runs the batch
// normalisation of amdmsm_batch_to_special over them (import_bases in normal form, one inversion per IMPORT_K records,
// then export_affine), its n affine records in `scratch`.
struct vec_opts {
    int mont, form, kernel_form;
};
vec_opts vec_opts_of(const amdmsm_opts *opts) {
    const int form = opts ? opts->out_form : AMDMSM_OUT_LIBFF;
    return {(opts && opts->scalars_plain) ? 0 : 1, form, form == AMDMSM_OUT_AFFINE ? (int)AMDMSM_OUT_LIBFF : form};
}
void vec_finish(const group_vtable *vt, hipStream_t st, const vec_opts &vo, uint32_t *d_xyz, size_t n, uint32_t *scratch) {
    if (vo.form != AMDMSM_OUT_AFFINE) return;
    vt->import_bases(st, d_xyz, (size_t)vt->el_words * 3, 0, n, scratch);
    vt->export_affine(st, scratch, n, d_xyz);
}

// A strided host vector of libff records: the stride a caller left out, and what a stride has to be
int vec_check_stride(amdmsm_ctx *ctx, const group_vtable *vt, size_t &stride_bytes, const char *what) {
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    if (stride_bytes == 0) stride_bytes = xyz_bytes;
    if (stride_bytes % rec_align(vt) || stride_bytes < xyz_bytes) return fail(ctx, AMDMSM_ERR_BAD_ARG, what);
    return AMDMSM_OK;
}
// records [first, first + m) of such a vector, through the staging buffer hb_src (which the caller has sized) into
// compact affine records at d_aff
int vec_upload(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, const void *points_xyz, size_t stride_bytes, int base_form,
               size_t first, size_t m, void *d_aff) {
    // the last record of a strided vector ends with its coordinates: nothing past them is read
    HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_src.p, (const char *)points_xyz + first * stride_bytes,
                                (m - 1) * stride_bytes + (size_t)vt->el_words * 12, hipMemcpyHostToDevice, st));
    vt->import_bases(st, (const uint32_t *)ctx->hb_src.p, stride_bytes / 4, base_form == AMDMSM_FORM_SPECIAL, m, (uint32_t *)d_aff);
    return AMDMSM_OK;
}

// the workspace slot of a call, and the end of the call in it
int slot_begin(amdmsm_ctx *ctx, hipStream_t st, size_t bytes, ws_slot *&slp) {
    const int slot_idx = (int)(ctx->next++ % (unsigned)ctx->depth);
    ws_slot &sl = ctx->slots[slot_idx];
    ctx->last_slot = slot_idx;
    if (sl.used) HIP_TRY(ctx, hipStreamWaitEvent(st, sl.done, 0));   // previous user of this slot
    slp = &sl;
    return ensure_ws(ctx, sl, bytes);
}
int slot_end(amdmsm_ctx *ctx, hipStream_t st, ws_slot &sl) {
    record(ctx, sl, 5, st);
    if (ctx->timing) sl.last_ticket = (long long)ctx->ticket++;
    sl.ev_valid = ctx->timing;
    HIP_TRY(ctx, hipEventRecord(sl.done, st));
    sl.used = true;
    return AMDMSM_OK;
}

// The chunk loop of scalar_mul_vec and fold_vec.  chunk(slot, off, m, first) enqueues elements [off, off + m) and, in
// the first chunk, records the marks 1 .. 3 between its passes.  Phase times of a timed call, through the MSM's timing
// calls: [0] import (host entry: with the upload), [1] table, [2] ladder, [3] normalisation / export (host entry: with
// the download) -- those four of the first chunk -- [4] the chunks after the first, [AMDMSM_PH_TOTAL] the call.
// h_out == nullptr, a device entry: the chunk has written the caller's vector and nothing waits for it.  Otherwise a
// host entry, whose chunk uploads into the staging buffers and writes fb.out: the results go down to h_out, and the
// stream is drained before the next chunk reuses the buffers.
template <class Chunk>
int vec_run_chunks(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, size_t ws_bytes, size_t n, size_t cn, void *h_out,
                   Chunk &&chunk) {
    const size_t xyz_bytes = (size_t)vt->el_words * 12;
    ws_slot *sl = nullptr;
    int rc = slot_begin(ctx, st, ws_bytes, sl);
    if (rc) return rc;
    record(ctx, *sl, 0, st);
    for (size_t off = 0; off < n; off += cn) {
        const size_t m = n - off < cn ? n - off : cn;
        rc = chunk(*sl, off, m, off == 0);
        if (rc) {
            if (h_out) (void)hipDeviceSynchronize();   // nothing of this call may still touch the staging buffers
            return rc;
        }
        if (h_out) HIP_TRY(ctx, hipMemcpyAsync((char *)h_out + off * xyz_bytes, ctx->fb.out.p, m * xyz_bytes, hipMemcpyDeviceToHost, st));
        if (off == 0) record(ctx, *sl, 4, st);
        if (h_out) HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return slot_end(ctx, st, *sl);
}

// one chunk on device-resident inputs: table, ladder and the results in the caller's form, the table scratch -- which
// the ladder no longer needs -- lent to vec_finish
int smv_chunk(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, const uint32_t *d_aff, const uint32_t *d_sc, size_t cn,
              uint32_t *d_out, const vec_opts &vo, ws_slot &sl, bool timed) {
    uint32_t *table = (uint32_t *)sl.ws, *tmp = (uint32_t *)((char *)sl.ws + smv_table_bytes(vt, cn));
    if (timed) record(ctx, sl, 1, st);
    vt->smv_table(st, d_aff, cn, tmp, table);
    if (timed) record(ctx, sl, 2, st);
    vt->smv_ladder(st, table, cn, d_sc, vo.mont, vo.kernel_form, d_out);
    if (timed) record(ctx, sl, 3, st);
    vec_finish(vt, st, vo, d_out, cn, tmp);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

// a group the library does not carry -- (MNT6, G2) -- is refused before anything else is looked at, the context included
#define SMV_REFUSE_UNKNOWN(ctx, curve, group) \
    if (!find_vt(curve, group)) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve/group")

int amdmsm_scalar_mul_vec_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, const void *d_scalars,
                                 size_t n, void *d_out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (n && (!d_points_affine || !d_scalars || !d_out_xyz)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (!n) return AMDMSM_OK;
    hipStream_t st = stream_of(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    const size_t ew = (size_t)vt->el_words, per = 2 * smv_table_bytes(vt, 1), cn = vec_chunk_points(per, 0, n, chunk_points);
    return vec_run_chunks(ctx, vt, st, cn * per, n, cn, nullptr, [&](ws_slot &sl, size_t off, size_t m, bool first) {
        return smv_chunk(ctx, vt, st, (const uint32_t *)d_points_affine + off * 2 * ew, (const uint32_t *)d_scalars + off * vt->fr_words,
                         m, (uint32_t *)d_out_xyz + off * 3 * ew, vo, sl, first);
    });
}

int amdmsm_scalar_mul_vec(amdmsm_ctx *ctx, int curve, int group, const void *points_xyz, size_t stride_bytes, int base_form,
                          const void *scalars, size_t n, void *out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    if (n && (!points_xyz || !scalars || !out_xyz)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    int rc = vec_check_stride(ctx, vt, stride_bytes, "point stride");
    if (rc || !n) return rc;
    hipStream_t st = ctx->stream;
    const vec_opts vo = vec_opts_of(opts);
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8, fr_bytes = (size_t)vt->fr_words * 4;
    const size_t per = 2 * smv_table_bytes(vt, 1), cn = vec_chunk_points(per, 0, n, chunk_points);
    rc = ensure_buf(ctx, ctx->hb_src, cn * stride_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, cn * aff_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_sc, cn * fr_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->fb.out, cn * xyz_bytes);
    if (rc) return rc;
    return vec_run_chunks(ctx, vt, st, cn * per, n, cn, out_xyz, [&](ws_slot &sl, size_t off, size_t m, bool first) {
        const int up = vec_upload(ctx, vt, st, points_xyz, stride_bytes, base_form, off, m, ctx->hb_aff.p);
        if (up) return up;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, (const char *)scalars + off * fr_bytes, m * fr_bytes, hipMemcpyHostToDevice, st));
        return smv_chunk(ctx, vt, st, (const uint32_t *)ctx->hb_aff.p, (const uint32_t *)ctx->hb_sc.p, m, (uint32_t *)ctx->fb.out.p, vo,
                         sl, first);
    });
}

// amdmsm_batch_exp on device-resident scalars, the results left in HBM: what a key generator whose Fr vectors are
// already there (amdmsm_fr_lincomb_device) calls instead of a download, the host entry and an upload.  The resident
// window table (fb_state) is the host entry's, under its reuse rule, and the kernels are its kernels; the results in
// special form come from vec_finish, the batch normalisation of the point-vector entries, its scratch a workspace slot.
// Enqueued on the caller's stream and not waited for: g and coeff are copied into pinned memory before the call returns.
int amdmsm_batch_exp_device(amdmsm_ctx *ctx, int curve, int group, size_t scalar_size, size_t window, const void *g_xyz,
                            const void *d_scalars, size_t n, const void *coeff, void *d_out_xyz, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    if (window < 1 || window > 22 || scalar_size < 1 || scalar_size > (size_t)find_vt(curve, group)->fr_words * 32)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "window / scalar_size");
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    if (vo.form != AMDMSM_OUT_LIBFF && vo.form != AMDMSM_OUT_AFFINE)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "out_form: AMDMSM_OUT_LIBFF or AMDMSM_OUT_AFFINE");
    if (!g_xyz || (n && (!d_scalars || !d_out_xyz))) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8, fr_bytes = (size_t)vt->fr_words * 4;
    if (n) {
        int rc = dev_check_aligned(ctx, "d_scalars", d_scalars, vt->fr_words % 4 ? 8 : 16);
        if (rc == AMDMSM_OK) rc = dev_check_aligned(ctx, "d_out_xyz", d_out_xyz, rec_align(vt));
        if (rc) return rc;
        if (dev_ranges_overlap(d_scalars, n * fr_bytes, d_out_xyz, n * xyz_bytes))
            return fail(ctx, AMDMSM_ERR_BAD_ARG, "d_out_xyz overlaps d_scalars");
    }
    const size_t outerc = (scalar_size + window - 1) / window;
    const size_t entries = outerc << window;
    hipStream_t st = stream_of(ctx, opts);
    fb_state &fb = ctx->fb;
    const bool same_table = fb.valid && fb.curve == curve && fb.group == group && fb.scalar_size == scalar_size &&
                            fb.window == window && memcmp(fb.g, g_xyz, xyz_bytes) == 0;
    int rc = ensure_buf(ctx, fb.small, 2 * xyz_bytes + outerc * xyz_bytes + 64);
    if (rc == AMDMSM_OK && !same_table) {
        fb.valid = false;
        rc = ensure_buf(ctx, fb.table, entries * xyz_bytes);
        if (rc == AMDMSM_OK) rc = ensure_buf(ctx, fb.table_aff, entries * aff_bytes);
    }
    if (rc) return rc;
    if (!fb.used) HIP_TRY(ctx, hipEventCreateWithFlags(&fb.used, hipEventDisableTiming));
    for (hipEvent_t &e : fb.uploaded) {
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (!fb.h_up) HIP_TRY(ctx, hipHostMalloc(&fb.h_up, fb_state::UP_BLOCKS * 2 * sizeof(fb.g), hipHostMallocDefault));
    char *d_g = (char *)fb.small.p, *d_cf = d_g + xyz_bytes, *d_go = d_cf + xyz_bytes;
    // the last call of this entry, on whatever stream: it may still read the table and the coefficient slot
    if (fb.used_valid) HIP_TRY(ctx, hipStreamWaitEvent(st, fb.used, 0));
    // From the first launch on, whatever way the call ends, `used` stands behind what it has enqueued: a call that fails
    // half way leaves kernels that read the table, and the next call on another stream has to wait for them too.
    struct used_guard {
        fb_state &fb;
        hipStream_t st;
        ~used_guard() {
            if (hipEventRecord(fb.used, st) == hipSuccess) fb.used_valid = true;
        }
    } mark_used{fb, st};
    ctx->aux_pending = false;
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[0], st));
    if (!same_table || coeff) {
        const unsigned blk = fb.up_next++ % fb_state::UP_BLOCKS;
        char *h_g = (char *)fb.h_up + (size_t)blk * 2 * sizeof(fb.g), *h_cf = h_g + sizeof(fb.g);
        if (fb.uploaded_valid[blk]) HIP_TRY(ctx, hipEventSynchronize(fb.uploaded[blk]));   // the copy out of this block, UP_BLOCKS uploads ago
        if (!same_table) {
            memcpy(h_g, g_xyz, xyz_bytes);
            HIP_TRY(ctx, hipMemcpyAsync(d_g, h_g, xyz_bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(fb.table.p, 0, entries * xyz_bytes, st));   // rows shorter than 2^window: infinity beyond
        }
        if (coeff) {
            memcpy(h_cf, coeff, fr_bytes);
            HIP_TRY(ctx, hipMemcpyAsync(d_cf, h_cf, fr_bytes, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(ctx, hipEventRecord(fb.uploaded[blk], st));
        fb.uploaded_valid[blk] = true;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[1], st));
    if (!same_table) {
        vt->fixed_base_exp(st, (const uint32_t *)d_g, (int)scalar_size, (int)window, nullptr, 0, 0, nullptr, AMDMSM_OUT_LIBFF,
                           (uint32_t *)d_go, (uint32_t *)fb.table.p, (uint32_t *)fb.table_aff.p, 1, nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[2], st));
    if (n) {
        vt->fixed_base_exp(st, (const uint32_t *)d_g, (int)scalar_size, (int)window, (const uint32_t *)d_scalars, n, vo.mont,
                           coeff ? (const uint32_t *)d_cf : nullptr, AMDMSM_OUT_LIBFF, (uint32_t *)d_go, (uint32_t *)fb.table.p,
                           (uint32_t *)fb.table_aff.p, 0, (uint32_t *)d_out_xyz);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[3], st));
    const bool normalise = n && vo.form == AMDMSM_OUT_AFFINE;
    if (normalise) {
        ws_slot *sl = nullptr;
        rc = slot_begin(ctx, st, n * aff_bytes, sl);
        if (rc) return rc;
        for (int i = 0; i < 5; ++i) record(ctx, *sl, i, st);   // a timed context: the whole slot time is normalisation
        vec_finish(vt, st, vo, (uint32_t *)d_out_xyz, n, (uint32_t *)sl->ws);
        HIP_TRY(ctx, hipGetLastError());
        rc = slot_end(ctx, st, *sl);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[4], st));
    ctx->aux_pending = true;
    ctx->aux_reused = same_table;
    ctx->aux_normalised = normalise;
    fb.valid = true;
    fb.curve = curve;
    fb.group = group;
    fb.scalar_size = scalar_size;
    fb.window = window;
    memcpy(fb.g, g_xyz, xyz_bytes);
    return AMDMSM_OK;
}

}  // extern "C"

// ---- fold of k point vectors by k shared scalars: out[i] = sum_j s_j * P_j[i] ---------------------------------------------
namespace {

// What a call runs: digit rows (two per scalar with the endomorphism split), windows per row, elements per chunk.  The
// split follows the permission rule of use_endomorphism without its cost model -- the table of phi(P) is the table of P
// with x scaled, so the 2 k half-length rows share half as many doublings at no other cost.  The workspace of a chunk is
// the digit rows, the k tables and one table's worth of scratch, which the k table passes use one after the other:
// (k + 1) * smv_entries compact affine records per element, which is what vec_chunk_points is given.
struct fold_plan {
    bool glv;
    int rows, W;
    size_t cn, ws_bytes;
};
fold_plan fold_make_plan(const group_vtable *vt, int k, size_t n, size_t chunk_points, const amdmsm_opts *opts) {
    fold_plan p;
    p.glv = endomorphism_permitted(vt, opts) != 0;
    p.rows = p.glv ? 2 * k : k;
    p.W = p.glv ? glv_windows(vt, 4) : vt->seg_windows;   // the ladder's 4-bit windows (msm_group.hip SMV_W)
    const size_t per = (size_t)(k + 1) * smv_table_bytes(vt, 1);
    p.cn = vec_chunk_points(per, FOLD_DIGIT_BYTES, n, chunk_points);
    p.ws_bytes = FOLD_DIGIT_BYTES + p.cn * per;
    return p;
}

// one chunk on device-resident inputs: the k tables (and, in the first chunk, the digit rows, which every chunk shares),
// the ladder and the results in the caller's form, the table scratch lent to vec_finish
int fold_chunk(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, const fold_plan &p, int k, const uint32_t *const *d_aff,
               size_t aff_off_words, const uint32_t *scalars, size_t cn, uint32_t *d_out, const vec_opts &vo, ws_slot &sl,
               bool first) {
    const size_t table_words = smv_table_bytes(vt, cn) / 4;
    uint32_t *digits = (uint32_t *)sl.ws, *tables = (uint32_t *)((char *)sl.ws + FOLD_DIGIT_BYTES), *tmp = tables + (size_t)k * table_words;
    if (first) {
        record(ctx, sl, 1, st);
        vt->fold_digits(st, scalars, k, vo.mont, p.glv ? 1 : 0, p.W, digits);
    }
    for (int j = 0; j < k; ++j) vt->smv_table(st, d_aff[j] + aff_off_words, cn, tmp, tables + (size_t)j * table_words);
    if (first) record(ctx, sl, 2, st);
    vt->fold_ladder(st, tables, cn, digits, p.rows, p.glv ? 1 : 0, p.W, vo.kernel_form, d_out);
    if (first) record(ctx, sl, 3, st);
    vec_finish(vt, st, vo, d_out, cn, tmp);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

// the argument rules both entries share; nothing is launched or written before they hold
int fold_check(amdmsm_ctx *ctx, int k, const void *const *vectors, const void *scalars, size_t n, const void *out) {
    if (k < 1 || k > FOLD_MAX_K) return fail(ctx, AMDMSM_ERR_BAD_ARG, "k = " + std::to_string(k) + ": 1 .. " + std::to_string(FOLD_MAX_K) + " vectors");
    if (!vectors) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer array");
    if (!n) return AMDMSM_OK;
    for (int j = 0; j < k; ++j)
        if (!vectors[j]) return fail(ctx, AMDMSM_ERR_BAD_ARG, "vector " + std::to_string(j) + ": null pointer");
    if (!scalars) return fail(ctx, AMDMSM_ERR_BAD_ARG, "scalars: null pointer");
    if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_plan_fold(int curve, int group, int k, size_t n, size_t chunk_points, int endomorphism, size_t out[5]) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return AMDMSM_ERR_UNSUPPORTED;
    if (!out || k < 1 || k > FOLD_MAX_K) return AMDMSM_ERR_BAD_ARG;
    amdmsm_opts o = AMDMSM_OPTS_INIT;
    o.endomorphism = endomorphism;
    const fold_plan p = fold_make_plan(vt, k, n, chunk_points, &o);
    out[0] = (size_t)p.rows;
    out[1] = (size_t)p.W;
    out[2] = p.glv ? 1 : 0;
    out[3] = p.cn;
    out[4] = p.ws_bytes;
    return AMDMSM_OK;
}

int amdmsm_fold_vec_device(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *d_points_affine, const void *scalars,
                           size_t n, void *d_out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = fold_check(ctx, k, d_points_affine, scalars, n, d_out_xyz);
    if (rc || !n) return rc;
    hipStream_t st = stream_of(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    const size_t ew = (size_t)vt->el_words;
    const fold_plan p = fold_make_plan(vt, k, n, chunk_points, opts);
    return vec_run_chunks(ctx, vt, st, p.ws_bytes, n, p.cn, nullptr, [&](ws_slot &sl, size_t off, size_t m, bool first) {
        return fold_chunk(ctx, vt, st, p, k, (const uint32_t *const *)d_points_affine, off * 2 * ew, (const uint32_t *)scalars, m,
                          (uint32_t *)d_out_xyz + off * 3 * ew, vo, sl, first);
    });
}

int amdmsm_fold_vec(amdmsm_ctx *ctx, int curve, int group, int k, const void *const *points_xyz, size_t stride_bytes, int base_form,
                    const void *scalars, size_t n, void *out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = vec_check_stride(ctx, vt, stride_bytes, "point stride");
    if (rc) return rc;
    rc = fold_check(ctx, k, points_xyz, scalars, n, out_xyz);
    if (rc || !n) return rc;
    hipStream_t st = ctx->stream;
    const vec_opts vo = vec_opts_of(opts);
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    const fold_plan p = fold_make_plan(vt, k, n, chunk_points, opts);
    rc = ensure_buf(ctx, ctx->hb_src, p.cn * stride_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, (size_t)k * p.cn * aff_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->fb.out, p.cn * xyz_bytes);
    if (rc) return rc;
    uint32_t *d_aff[FOLD_MAX_K];
    for (int j = 0; j < k; ++j) d_aff[j] = (uint32_t *)((char *)ctx->hb_aff.p + (size_t)j * p.cn * aff_bytes);
    return vec_run_chunks(ctx, vt, st, p.ws_bytes, n, p.cn, out_xyz, [&](ws_slot &sl, size_t off, size_t m, bool first) {
        // vector after vector through the one staging buffer, in stream order
        for (int j = 0; j < k; ++j) {
            const int up = vec_upload(ctx, vt, st, points_xyz[j], stride_bytes, base_form, off, m, d_aff[j]);
            if (up) return up;
        }
        return fold_chunk(ctx, vt, st, p, k, d_aff, 0, (const uint32_t *)scalars, m, (uint32_t *)ctx->fb.out.p, vo, sl, first);
    });
}

}  // extern "C"

// ---- radix-2 FFT over a point vector: out[j] = sum_i w^(i j) P_i ------------------------------------------------------------
namespace {

// log2 n autosorting stages of n / 2 butterflies each (group_vtable::fft_butterfly).  A stage reads the vector as compact
// affine records and writes libff records; the batch normalisation of vec_finish (import_bases in normal form) brings
// them back to compact affine for the next stage, into the other of two vectors.  The part of the workspace that is
// linear in n is those two vectors and the vector of libff records; the part that scales with the chunk is, per
// butterfly, smv_table's 2 * smv_entries records and the gathered B operand the table is built from: that part is what
// vec_chunk_points is given, a chunk being at most the n / 2 butterflies of a stage.
constexpr size_t FFT_MAX_N = (size_t)1 << 28;
constexpr size_t CALL_MAX_MARKS = (size_t)1 << 16;
struct fft_plan {
    int stages;
    size_t cn, chunk_bytes, off_a, off_b, off_xyz, off_chunk, ws_bytes;
};
size_t fft_chunk_bytes(const group_vtable *vt, size_t cn) { return 2 * smv_table_bytes(vt, cn) + cn * (size_t)vt->el_words * 8; }
fft_plan fft_make_plan(const group_vtable *vt, size_t n, size_t chunk_points) {
    fft_plan p = {};
    while (((size_t)2 << p.stages) <= n) ++p.stages;
    p.cn = vec_chunk_points(fft_chunk_bytes(vt, 1), 0, n / 2, chunk_points);
    p.chunk_bytes = fft_chunk_bytes(vt, p.cn);
    const size_t aff = align_up(n * (size_t)vt->el_words * 8, 256), xyz = align_up(n * (size_t)vt->el_words * 12, 256);
    p.off_a = 0;
    p.off_b = aff;
    p.off_xyz = 2 * aff;
    p.off_chunk = 2 * aff + xyz;
    p.ws_bytes = p.off_chunk + p.chunk_bytes;
    return p;
}

// phase mark of a timed call (amdmsm_ctx::call_ev)
void call_mark(amdmsm_ctx *ctx, hipStream_t st, int phase, bool last = false) {
    if (!ctx->timing) return;
    if (ctx->call_marks >= CALL_MAX_MARKS && !last) return;   // the time stays with the phase of the mark before
    if (ctx->call_marks == ctx->call_ev.size()) {
        hipEvent_t e = nullptr;
        if (timing_event(&e) != hipSuccess) return;
        ctx->call_ev.push_back(e);
        ctx->call_phase.push_back(0);
    }
    (void)hipEventRecord(ctx->call_ev[ctx->call_marks], st);
    ctx->call_phase[ctx->call_marks++] = (unsigned char)phase;
}

// the argument rules all entries share; nothing is launched or written before they hold
int fft_check(amdmsm_ctx *ctx, size_t n, const void *points, const void *twiddles, const void *out) {
    if (n & (n - 1)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "n = " + std::to_string(n) + " is not a power of two");
    if (n > FFT_MAX_N) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n = " + std::to_string(n) + ": at most 2^28 points");
    if (!n) return AMDMSM_OK;
    if (!points) return fail(ctx, AMDMSM_ERR_BAD_ARG, "points: null pointer");
    if (!twiddles && n > 2) return fail(ctx, AMDMSM_ERR_BAD_ARG, "twiddles: null pointer");
    if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    return AMDMSM_OK;
}

// the stages on device-resident inputs, n >= 1: d_in is read only (it may be the workspace's first vector), d_out
// receives n records in `form`
int fft_stages(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, const fft_plan &p, const uint32_t *d_in,
               const uint32_t *d_tw, size_t n, uint32_t *d_out, const vec_opts &vo, char *ws) {
    uint32_t *buf_a = (uint32_t *)(ws + p.off_a), *buf_b = (uint32_t *)(ws + p.off_b), *xyz = (uint32_t *)(ws + p.off_xyz);
    uint32_t *gathered = (uint32_t *)(ws + p.off_chunk);
    uint32_t *table = gathered + p.cn * (size_t)vt->el_words * 2, *tmp = table + smv_table_bytes(vt, p.cn) / 4;
    const size_t xyz_words = (size_t)vt->el_words * 3, half = n / 2;
    if (n == 1) {   // the point itself, in special form -- which is a libff record too
        call_mark(ctx, st, 3);
        vt->export_affine(st, d_in, 1, d_out);
        HIP_TRY(ctx, hipGetLastError());
        return AMDMSM_OK;
    }
    const uint32_t *cur = d_in;
    for (int t = 0; t < p.stages; ++t) {
        const int rsh = p.stages - 1 - t;
        const bool last = t == p.stages - 1;
        uint32_t *dst = last ? d_out : xyz;
        uint32_t *next = cur == buf_a ? buf_b : buf_a;
        for (size_t b0 = 0; b0 < half; b0 += p.cn) {
            const size_t m = half - b0 < p.cn ? half - b0 : p.cn;
            if (t == 0) {   // every twiddle is 1
                call_mark(ctx, st, 2);
                vt->fft_butterfly(st, nullptr, m, cur, b0, rsh, d_tw, vo.mont, half, dst);
            } else {
                call_mark(ctx, st, 1);
                vt->fft_gather(st, cur, b0, m, rsh, gathered);
                vt->smv_table(st, gathered, m, tmp, table);
                call_mark(ctx, st, 2);
                vt->fft_butterfly(st, table, m, cur, b0, rsh, d_tw, vo.mont, half, dst);
            }
        }
        call_mark(ctx, st, 3);
        if (!last) {
            vt->import_bases(st, dst, xyz_words, 0, n, next);
            cur = next;
        } else {
            vec_finish(vt, st, vo, dst, n, next);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return AMDMSM_OK;
}

// the slot and the first mark of a call whose phases are marked (group_fft, the Fr entries); the last mark and the end of
// the call
int call_begin(amdmsm_ctx *ctx, hipStream_t st, size_t ws_bytes, ws_slot *&sl) {
    const int rc = slot_begin(ctx, st, ws_bytes, sl);
    if (rc) return rc;
    ctx->call_marks = 0;
    ctx->call_ticket = -1;
    record(ctx, *sl, 0, st);
    call_mark(ctx, st, 0);
    return AMDMSM_OK;
}
int call_end(amdmsm_ctx *ctx, hipStream_t st, ws_slot &sl, int last_phase = 3) {
    call_mark(ctx, st, last_phase, true);
    if (ctx->timing) ctx->call_ticket = (long long)ctx->ticket;   // the ticket slot_end hands out
    return slot_end(ctx, st, sl);
}

}   // namespace

extern "C" {

int amdmsm_fr_modulus(int curve, int group, void *r_plain) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return AMDMSM_ERR_UNSUPPORTED;
    if (!r_plain) return AMDMSM_ERR_BAD_ARG;
    memcpy(r_plain, vt->fr_modulus, (size_t)vt->fr_words * 4);
    return AMDMSM_OK;
}

int amdmsm_plan_group_fft(int curve, int group, size_t n, size_t chunk_points, size_t out[6]) {
    const group_vtable *vt = find_vt(curve, group);
    if (!vt) return AMDMSM_ERR_UNSUPPORTED;
    if (!out || (n & (n - 1))) return AMDMSM_ERR_BAD_ARG;
    if (n > FFT_MAX_N) return AMDMSM_ERR_TOO_LARGE;
    const fft_plan p = fft_make_plan(vt, n, chunk_points);
    out[0] = (size_t)p.stages;
    out[1] = p.stages > 1 ? (size_t)p.stages - 1 : 0;
    out[2] = n / 2 * out[1];
    out[3] = p.cn;
    out[4] = p.ws_bytes;
    out[5] = p.chunk_bytes;
    return AMDMSM_OK;
}

int amdmsm_group_fft_device(amdmsm_ctx *ctx, int curve, int group, const void *d_points_affine, size_t n, const void *d_twiddles,
                            void *d_out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = fft_check(ctx, n, d_points_affine, d_twiddles, d_out_xyz);
    if (rc || !n) return rc;
    hipStream_t st = stream_of(ctx, opts);
    const fft_plan p = fft_make_plan(vt, n, chunk_points);
    ws_slot *sl = nullptr;
    rc = call_begin(ctx, st, p.ws_bytes, sl);
    if (rc) return rc;
    rc = fft_stages(ctx, vt, st, p, (const uint32_t *)d_points_affine, (const uint32_t *)d_twiddles, n, (uint32_t *)d_out_xyz,
                    vec_opts_of(opts), (char *)sl->ws);
    if (rc) return rc;
    return call_end(ctx, st, *sl);
}

int amdmsm_group_fft(amdmsm_ctx *ctx, int curve, int group, const void *points_xyz, size_t stride_bytes, int base_form, size_t n,
                     const void *twiddles, void *out_xyz, size_t chunk_points, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    int rc = vec_check_stride(ctx, vt, stride_bytes, "point stride");
    if (rc) return rc;
    rc = fft_check(ctx, n, points_xyz, twiddles, out_xyz);
    if (rc || !n) return rc;
    hipStream_t st = ctx->stream;
    const size_t xyz_bytes = (size_t)vt->el_words * 12, fr_bytes = (size_t)vt->fr_words * 4;
    const fft_plan p = fft_make_plan(vt, n, chunk_points);
    // the records go up through the staging buffer a piece at a time: two points per butterfly of a chunk
    const size_t piece = n < 2 * p.cn || !p.cn ? n : 2 * p.cn;
    rc = ensure_buf(ctx, ctx->hb_src, piece * stride_bytes);
    if (rc == AMDMSM_OK && n > 2) rc = ensure_buf(ctx, ctx->hb_sc, n / 2 * fr_bytes);
    ws_slot *sl = nullptr;
    if (rc == AMDMSM_OK) rc = call_begin(ctx, st, p.ws_bytes, sl);
    if (rc) return rc;
    char *ws = (char *)sl->ws;
    uint32_t *d_in = (uint32_t *)(ws + p.off_a), *d_res = (uint32_t *)(ws + p.off_xyz);
    for (size_t off = 0; off < n; off += piece) {
        const size_t m = n - off < piece ? n - off : piece;
        rc = vec_upload(ctx, vt, st, points_xyz, stride_bytes, base_form, off, m, d_in + off * (size_t)vt->el_words * 2);
        if (rc) return rc;
        // the next piece reuses the staging buffer
        if (off + piece < n) HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (n > 2) HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, twiddles, n / 2 * fr_bytes, hipMemcpyHostToDevice, st));
    rc = fft_stages(ctx, vt, st, p, d_in, (const uint32_t *)ctx->hb_sc.p, n, d_res, vec_opts_of(opts), ws);
    if (rc) {
        (void)hipDeviceSynchronize();   // nothing of this call may still touch the staging buffers
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, d_res, n * xyz_bytes, hipMemcpyDeviceToHost, st));
    rc = call_end(ctx, st, *sl);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return rc;
}

}  // extern "C"

// ---- segmented MSM: out[j] = sum of s_i * P_i over segment j ------------------------------------------------------------
namespace {

// Terms one accumulation lane adds in a row: a longer segment is cut into slices of this many terms, whose window sums
// are added before the Horner chain, so that one long segment among short ones does not hold its 65 .. 97 lanes for the
// whole pass.
constexpr size_t SEG_CHAIN_CAP = 512;
// Segments of at least this many terms take the single-MSM route when the caller passes long_from = 0.  Measured
// (profiles/segmented_msm.txt): a lone segment of 2^8 .. 2^14 terms is faster on the single-MSM route
// at every size -- one segment cannot fill the device -- so that sweep gives no default; the rule is the length at which
// a segment costs the segment pass of a full device (2^10 segments of 256 terms: 19 / 158 / 32 ns per term for
// alt_bn128 G1 / bls12_377 G2 / mnt4 G1) what a single MSM of that length costs (0.49 / 2.1 / 1.35 ms): 2^14.6 / 2^13.7 /
// 2^15.3 terms, rounded down, keyed by the words per coordinate (8 / 24 / 10 measured, the others by width).
size_t seg_long_from_default(const group_vtable *vt) { return vt->el_words > 12 ? (size_t)1 << 13 : (size_t)1 << 14; }

// a run of consecutive short segments worked through in one pass: segments [j0, j1), terms [t0, t0 + ct), ns slices;
// desc: word offset of its descriptors (ns slices of 4 words, then j1 - j0 + 1 words of seg_first)
struct seg_chunk {
    size_t j0, j1, t0, ct, ns, desc;
};
struct seg_layout {
    size_t table, digits, sums, winsum, norm, total;   // byte offsets inside a chunk's area
};
seg_layout seg_chunk_layout(const group_vtable *vt, bool shared, size_t ct, size_t ns, size_t mc) {
    const size_t aff_bytes = (size_t)vt->el_words * 8, D = (size_t)vt->seg_windows;
    seg_layout l;
    size_t off = 0;
    l.table = off;
    if (!shared) off = align_up(off + 2 * smv_table_bytes(vt, ct), 256);   // table and its scratch
    l.digits = off;
    off = align_up(off + ct * (size_t)vt->seg_digit_stride, 256);
    l.sums = off;
    off = align_up(off + ns * D * (size_t)vt->el_words * 16, 256);
    l.winsum = off;
    off = align_up(off + mc * D * (size_t)vt->el_words * 12, 256);
    l.norm = off;
    off = align_up(off + mc * aff_bytes, 256);
    l.total = off;
    return l;
}

// the argument rules of both entries; nothing is launched or written before they hold
int seg_check(amdmsm_ctx *ctx, const void *bases, size_t n_bases, const void *scalars, size_t n_terms, const uint64_t *offsets,
              size_t m, unsigned flags, const void *out) {
    if (flags & ~(unsigned)AMDMSM_SEG_SHARED_BASES) return fail(ctx, AMDMSM_ERR_BAD_ARG, "unknown flag");
    if (!m) return AMDMSM_OK;
    if (!offsets || !out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    const bool shared = (flags & AMDMSM_SEG_SHARED_BASES) != 0;
    if (!shared && n_bases != n_terms) return fail(ctx, AMDMSM_ERR_BAD_ARG, "n_bases must equal n_terms without AMDMSM_SEG_SHARED_BASES");
    for (size_t j = 0; j < m; ++j) {
        if (offsets[j + 1] < offsets[j]) return fail(ctx, AMDMSM_ERR_BAD_ARG, "segment " + std::to_string(j) + ": offsets decrease");
        if (shared && offsets[j + 1] - offsets[j] > n_bases)
            return fail(ctx, AMDMSM_ERR_BAD_ARG, "segment " + std::to_string(j) + ": longer than the shared base vector");
    }
    if (offsets[m] > n_terms) return fail(ctx, AMDMSM_ERR_BAD_ARG, "segment " + std::to_string(m - 1) + ": offsets[m] > n_terms");
    if (offsets[m] > offsets[0] && (!bases || !scalars)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    return AMDMSM_OK;
}

// Device-resident inputs, arguments checked.  The short segments run chunk by chunk -- whole segments, as many as keep
// table, table scratch, digits and window sums inside SMV_WS_BUDGET (a segment too long for that alone is a chunk of its
// own) -- in the call's workspace slot; a segment of long_from terms or more ends the chunk in front of it and is run
// afterwards through msm_device_ranges, straight into its own out[j].  Phase times of a timed call: [0] table (the
// shared one, or the first chunk's), [1] digits, [2] accumulation and slice sums, [3] Horner -- of the first chunk --
// [4] its normalisation and the chunks after it, [AMDMSM_PH_TOTAL] the short pass; every long segment is a timed MSM of
// its own.
int seg_device_impl(amdmsm_ctx *ctx, const group_vtable *vt, const uint32_t *d_bases, size_t n_bases, const uint32_t *d_scalars,
                    const uint64_t *offsets, size_t m, unsigned flags, size_t long_from, uint32_t *d_out, const amdmsm_opts *opts) {
    hipStream_t st = stream_of(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    const bool shared = (flags & AMDMSM_SEG_SHARED_BASES) != 0;
    if (!long_from) long_from = seg_long_from_default(vt);
    const size_t ew = (size_t)vt->el_words, xyzw = 3 * ew, affw = 2 * ew, frw = (size_t)vt->fr_words;
    const size_t cap_terms = ctx->seg_chunk_terms;

    std::vector<seg_chunk> chunks;
    std::vector<size_t> longs;
    std::vector<uint32_t> desc;
    size_t chunk_area = 0;
    auto close = [&](seg_chunk &c, size_t j1) {
        c.j1 = j1;
        if (c.j1 == c.j0) return;
        // descriptors: the slices, then seg_first (padded to whole 16-byte records)
        c.desc = desc.size();
        size_t ns = 0;
        for (size_t j = c.j0; j < c.j1; ++j) {
            const size_t len = (size_t)(offsets[j + 1] - offsets[j]);
            for (size_t k = 0; k < len; k += SEG_CHAIN_CAP) {
                const size_t a = (size_t)offsets[j] - c.t0 + k, e = std::min(a + SEG_CHAIN_CAP, (size_t)offsets[j + 1] - c.t0);
                desc.insert(desc.end(), {(uint32_t)a, (uint32_t)e, (uint32_t)(shared ? k : a), 0u});
                ++ns;
            }
        }
        size_t first = 0;
        for (size_t j = c.j0; j < c.j1; ++j) {
            desc.push_back((uint32_t)first);
            first += ((size_t)(offsets[j + 1] - offsets[j]) + SEG_CHAIN_CAP - 1) / SEG_CHAIN_CAP;
        }
        desc.push_back((uint32_t)first);
        while (desc.size() % 4) desc.push_back(0u);
        c.ns = ns;
        chunk_area = std::max(chunk_area, seg_chunk_layout(vt, shared, c.ct, c.ns, c.j1 - c.j0).total);
        chunks.push_back(c);
    };
    seg_chunk cur{0, 0, m ? (size_t)offsets[0] : 0, 0, 0, 0};
    for (size_t j = 0; j < m; ++j) {
        const size_t len = (size_t)(offsets[j + 1] - offsets[j]);
        if (len >= long_from) {
            close(cur, j);
            longs.push_back(j);
            cur = seg_chunk{j + 1, j + 1, (size_t)offsets[j + 1], 0, 0, 0};
            continue;
        }
        if (len >= ((size_t)1 << 31)) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "segment " + std::to_string(j) + ": too long for the segment pass");
        const size_t sl = (len + SEG_CHAIN_CAP - 1) / SEG_CHAIN_CAP;
        if (cur.j1 > cur.j0 && ((cap_terms && cur.ct + len > cap_terms) || cur.ct + len >= ((size_t)1 << 31) ||
                                seg_chunk_layout(vt, shared, cur.ct + len, cur.ns + sl, j + 1 - cur.j0).total > SMV_WS_BUDGET)) {
            close(cur, j);
            cur = seg_chunk{j, j, (size_t)offsets[j], 0, 0, 0};
        }
        cur.ct += len;
        cur.ns += sl;
        cur.j1 = j + 1;
    }
    close(cur, cur.j1);

    if (!chunks.empty()) {
        // workspace: descriptors of every chunk | shared table | one chunk's area (the shared table's scratch lies there too)
        const size_t desc_bytes = align_up(desc.size() * 4, 256);
        const size_t shared_bytes = shared ? align_up(smv_table_bytes(vt, n_bases), 256) : 0;
        if (shared) chunk_area = std::max(chunk_area, smv_table_bytes(vt, n_bases));
        ws_slot *sl = nullptr;
        int rc = slot_begin(ctx, st, desc_bytes + shared_bytes + chunk_area, sl);
        if (rc) return rc;
        char *ws = (char *)sl->ws, *area = ws + desc_bytes + shared_bytes;
        const uint32_t *d_desc = (const uint32_t *)ws;
        uint32_t *shared_table = (uint32_t *)(ws + desc_bytes);
        // the descriptors go up through pinned memory, so that the call stays asynchronous
        if (ctx->seg_copied) HIP_TRY(ctx, hipEventSynchronize(ctx->seg_copied));
        else HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->seg_copied, hipEventDisableTiming));
        if (ctx->seg_host_bytes < desc.size() * 4) {
            if (ctx->seg_host) HIP_TRY(ctx, hipHostFree(ctx->seg_host));
            ctx->seg_host = nullptr;
            ctx->seg_host_bytes = 0;
            HIP_TRY(ctx, hipHostMalloc(&ctx->seg_host, desc.size() * 4 * 2, hipHostMallocDefault));
            ctx->seg_host_bytes = desc.size() * 4 * 2;
        }
        memcpy(ctx->seg_host, desc.data(), desc.size() * 4);
        HIP_TRY(ctx, hipMemcpyAsync(ws, ctx->seg_host, desc.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipEventRecord(ctx->seg_copied, st));
        record(ctx, *sl, 0, st);
        if (shared) vt->smv_table(st, d_bases, n_bases, (uint32_t *)area, shared_table);
        bool first = true;
        for (const seg_chunk &c : chunks) {
            const size_t mc = c.j1 - c.j0;
            const seg_layout l = seg_chunk_layout(vt, shared, c.ct, c.ns, mc);
            uint32_t *table = shared ? shared_table : (uint32_t *)(area + l.table);
            uint32_t *digits = (uint32_t *)(area + l.digits), *sums = (uint32_t *)(area + l.sums);
            uint32_t *winsum = (uint32_t *)(area + l.winsum), *norm = (uint32_t *)(area + l.norm);
            uint32_t *out = d_out + c.j0 * xyzw;
            if (!shared) vt->smv_table(st, d_bases + c.t0 * affw, c.ct, (uint32_t *)(area + l.table + smv_table_bytes(vt, c.ct)), table);
            if (first) record(ctx, *sl, 1, st);
            vt->seg_digits(st, d_scalars + c.t0 * frw, c.ct, vo.mont, digits);
            if (first) record(ctx, *sl, 2, st);
            vt->seg_accumulate(st, table, shared ? n_bases : c.ct, digits, d_desc + c.desc, c.ns, sums);
            vt->seg_fold(st, sums, d_desc + c.desc + 4 * c.ns, mc, winsum);
            if (first) record(ctx, *sl, 3, st);
            vt->seg_horner(st, winsum, mc, vo.kernel_form, out);
            if (first) record(ctx, *sl, 4, st);
            vec_finish(vt, st, vo, out, mc, norm);
            HIP_TRY(ctx, hipGetLastError());
            first = false;
        }
        rc = slot_end(ctx, st, *sl);
        if (rc) return rc;
    }
    for (size_t j : longs) {
        const size_t len = (size_t)(offsets[j + 1] - offsets[j]);
        const int rc = msm_device_ranges(ctx, vt, shared ? d_bases : d_bases + (size_t)offsets[j] * affw,
                                         d_scalars + (size_t)offsets[j] * frw, len, d_out + j * xyzw, opts);
        if (rc) return rc;
    }
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_set_segments_chunk_terms(amdmsm_ctx *ctx, size_t chunk_terms) {
    if (!ctx) return AMDMSM_ERR_BAD_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    ctx->seg_chunk_terms = chunk_terms;
    return AMDMSM_OK;
}

int amdmsm_msm_device_segments(amdmsm_ctx *ctx, int curve, int group, const void *d_bases_affine, size_t n_bases,
                               const void *d_scalars, size_t n_terms, const uint64_t *offsets, size_t m, unsigned flags,
                               size_t long_from, void *d_out, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const int rc = seg_check(ctx, d_bases_affine, n_bases, d_scalars, n_terms, offsets, m, flags, d_out);
    if (rc || !m) return rc;
    return seg_device_impl(ctx, vt, (const uint32_t *)d_bases_affine, n_bases, (const uint32_t *)d_scalars, offsets, m, flags,
                           long_from, (uint32_t *)d_out, opts);
}

int amdmsm_multi_exp_segments(amdmsm_ctx *ctx, int curve, int group, const void *bases_xyz, size_t base_stride_bytes,
                              int base_form, size_t n_bases, const void *scalars, size_t n_terms, const uint64_t *offsets,
                              size_t m, unsigned flags, size_t long_from, void *out, const amdmsm_opts *opts) {
    SMV_REFUSE_UNKNOWN(ctx, curve, group);
    GET_VT(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8, fr_bytes = (size_t)vt->fr_words * 4;
    int rc = vec_check_stride(ctx, vt, base_stride_bytes, "base stride");
    if (rc) return rc;
    rc = seg_check(ctx, bases_xyz, n_bases, scalars, n_terms, offsets, m, flags, out);
    if (rc || !m) return rc;
    // only the terms some segment names are staged: offsets are rebased to the first of them
    const bool shared = (flags & AMDMSM_SEG_SHARED_BASES) != 0;
    const size_t t0 = (size_t)offsets[0], nt = (size_t)offsets[m] - t0;
    std::vector<uint64_t> offs(m + 1);
    size_t longest = 0;
    for (size_t j = 0; j <= m; ++j) {
        offs[j] = offsets[j] - t0;
        if (j) longest = std::max(longest, (size_t)(offs[j] - offs[j - 1]));
    }
    const size_t b0 = shared ? 0 : t0, nb = shared ? longest : nt;   // the bases in use
    hipStream_t st = ctx->stream;
    amdmsm_opts o = opts_or_default(opts);
    o.stream = nullptr;
    rc = ensure_buf(ctx, ctx->hb_src, nb ? nb * base_stride_bytes : 16);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, nb ? nb * aff_bytes : 16);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_sc, nt ? nt * fr_bytes : 16);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->fb.out, m * xyz_bytes);
    if (rc) return rc;
    if (nb) {
        rc = vec_upload(ctx, vt, st, bases_xyz, base_stride_bytes, base_form, b0, nb, ctx->hb_aff.p);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hb_sc.p, (const char *)scalars + t0 * fr_bytes, nt * fr_bytes, hipMemcpyHostToDevice, st));
    }
    rc = seg_device_impl(ctx, vt, (const uint32_t *)ctx->hb_aff.p, nb, (const uint32_t *)ctx->hb_sc.p, offs.data(), m, flags,
                         long_from, (uint32_t *)ctx->fb.out.p, &o);
    // the results reach the caller's array only when the whole call has succeeded
    std::vector<char> h_out(m * xyz_bytes);
    hipError_t e = hipSuccess;
    if (rc == AMDMSM_OK) e = hipMemcpyAsync(h_out.data(), ctx->fb.out.p, m * xyz_bytes, hipMemcpyDeviceToHost, st);
    if (rc == AMDMSM_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    if (rc || e != hipSuccess) {
        (void)hipDeviceSynchronize();   // nothing of this call may still touch the staging buffers
        return rc ? rc : fail(ctx, AMDMSM_ERR_HIP, hipGetErrorString(e));
    }
    memcpy(out, h_out.data(), m * xyz_bytes);
    return AMDMSM_OK;
}

}  // extern "C"

// ---- radix-2 FFT over a vector of Fr scalars: out[j] = post^j scale sum_i pre^i a_i w^(i j) --------------------------------
namespace {

using fr_getter = const fr_vtable *(*)();
const fr_vtable *find_frvt(int curve) {
    static const fr_getter getters[] = {frvt_alt_bn128, frvt_bls12_377, frvt_bw6_761, frvt_bls12_381, frvt_mnt4, frvt_mnt6};
    for (fr_getter g : getters) {
        if (!g) continue;
        const fr_vtable *v = g();
        if (v->curve == curve) return v;
    }
    return nullptr;
}

// The host's share of the arithmetic: a handful of Montgomery products on 32-bit words (the root check, the squarings
// behind the power tables), on the constants the field's unit exports.  Operands are words of the field's width;
// a canonical result for canonical operands, some value below 2^(32 words) for any others.
struct fr_rec {
    uint32_t v[FR_MAX_WORDS] = {};
};
fr_rec fr_mul(const fr_vtable *f, const fr_rec &a, const fr_rec &b) {
    const int N = f->words;
    const uint32_t *p = f->modulus;
    uint32_t t[FR_MAX_WORDS + 2] = {};
    for (int i = 0; i < N; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < N; ++j) {
            const uint64_t s = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        uint64_t s = (uint64_t)t[N] + c;
        t[N] = (uint32_t)s;
        t[N + 1] = (uint32_t)(s >> 32);
        const uint32_t m = t[0] * f->inv;
        c = ((uint64_t)m * p[0] + t[0]) >> 32;
        for (int j = 1; j < N; ++j) {
            s = (uint64_t)m * p[j] + t[j] + c;
            t[j - 1] = (uint32_t)s;
            c = s >> 32;
        }
        s = (uint64_t)t[N] + c;
        t[N - 1] = (uint32_t)s;
        t[N] = t[N + 1] + (uint32_t)(s >> 32);
        t[N + 1] = 0;
    }
    bool ge = t[N] != 0;
    if (!ge) {
        ge = true;
        for (int j = N - 1; j >= 0; --j) {
            if (t[j] != p[j]) {
                ge = t[j] > p[j];
                break;
            }
        }
    }
    fr_rec r;
    uint64_t borrow = 0;
    for (int j = 0; j < N; ++j) {
        const uint64_t d = (uint64_t)t[j] - (ge ? p[j] : 0) - borrow;
        r.v[j] = (uint32_t)d;
        borrow = (d >> 63) & 1u;
    }
    return r;
}
fr_rec fr_from_words(const fr_vtable *f, const uint32_t *w) {
    fr_rec r;
    memcpy(r.v, w, (size_t)f->words * 4);
    return r;
}
bool fr_same(const fr_vtable *f, const fr_rec &a, const fr_rec &b) { return memcmp(a.v, b.v, (size_t)f->words * 4) == 0; }
// a caller's record as a Montgomery residue
fr_rec fr_read(const fr_vtable *f, const void *rec, bool plain) {
    const fr_rec r = fr_from_words(f, (const uint32_t *)rec);
    return plain ? fr_mul(f, r, fr_from_words(f, f->r2)) : r;
}
fr_rec fr_small(uint32_t k) {
    fr_rec r;
    r.v[0] = k;
    return r;
}
// out of Montgomery form: the product with the integer 1
fr_rec fr_from_mont(const fr_vtable *f, const fr_rec &x) { return fr_mul(f, x, fr_small(1)); }
// r - x word by word, x <= r: r - 1 in either form (x = 1, x = R mod r), the Fermat exponent r - 2
fr_rec fr_r_minus(const fr_vtable *f, const fr_rec &x) {
    fr_rec d;
    uint64_t borrow = 0;
    for (int j = 0; j < f->words; ++j) {
        const uint64_t w = (uint64_t)f->modulus[j] - x.v[j] - borrow;
        d.v[j] = (uint32_t)w;
        borrow = (w >> 63) & 1u;
    }
    return d;
}
// an environment switch: set, not empty and not "0"
bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}
// base^(2^(shift + b)), b < FR_POW_TABLE, packed records of the field's width: what fr_vtable::powers takes for the
// powers of base^(2^shift)
std::vector<uint32_t> fr_pow_table(const fr_vtable *f, fr_rec x, int shift) {
    std::vector<uint32_t> t((size_t)FR_POW_TABLE * f->words);
    for (int b = 0; b < shift; ++b) x = fr_mul(f, x, x);
    for (int b = 0; b < FR_POW_TABLE; ++b) {
        memcpy(&t[(size_t)b * f->words], x.v, (size_t)f->words * 4);
        x = fr_mul(f, x, x);
    }
    return t;
}

constexpr size_t FR_FFT_MAX_N = (size_t)1 << 28;
int log2_exact(size_t n) {
    int l = 0;
    while (((size_t)1 << l) < n) ++l;
    return l;
}

// The passes of a transform: `tile` stages each, the last one the rest.  The workspace: one vector, the four vectors of
// powers of pre and post, and behind them the second vector that only an in-place call of an odd number of passes
// above one needs (frfft_ws_bytes).
struct frfft_plan {
    int log_n = 0, tile = 0, passes = 1, t_first = 0, t_last = 0;
    size_t rec = 0, vec = 0, off_w2 = 0, off_pre_col = 0, off_pre_row = 0, off_post_col = 0, off_post_row = 0, ws_all = 0, ws_plain = 0;
};
int frfft_make_plan(const fr_vtable *f, size_t n, int tile_log2, frfft_plan &p) {
    if (tile_log2 && (tile_log2 < FR_TILE_MIN || tile_log2 > FR_TILE_MAX)) return AMDMSM_ERR_BAD_ARG;
    p.log_n = log2_exact(n ? n : 1);
    p.tile = tile_log2 ? tile_log2 : FR_TILE_DEFAULT;
    p.passes = p.log_n ? (p.log_n + p.tile - 1) / p.tile : 1;
    p.t_first = std::min(p.tile, p.log_n);
    p.t_last = p.log_n - (p.passes - 1) * p.tile;
    p.rec = (size_t)f->words * 4;
    p.vec = align_up((n ? n : 1) * p.rec, 256);
    p.off_pre_col = p.vec;
    p.off_pre_row = p.off_pre_col + align_up((n >> p.t_first) * p.rec, 256);
    p.off_post_col = p.off_pre_row + align_up(((size_t)1 << p.t_first) * p.rec, 256);
    p.off_post_row = p.off_post_col + align_up((n >> p.t_last) * p.rec, 256);
    p.off_w2 = p.off_post_row + align_up(((size_t)1 << p.t_last) * p.rec, 256);
    p.ws_plain = p.off_w2;           // without the second vector
    p.ws_all = p.off_w2 + p.vec;
    return AMDMSM_OK;
}

bool frfft_third(const frfft_plan &p, bool in_place) { return in_place && p.passes > 1 && p.passes % 2 == 1; }
size_t frfft_ws_bytes(const frfft_plan &p, bool in_place) { return frfft_third(p, in_place) ? p.ws_all : p.ws_plain; }

// what a call is given, as Montgomery residues
struct frfft_params {
    bool plain = false, has_pre = false, has_post = false, has_scale = false;
    bool mont_in = false, mont_out = false;   // plain: the records of this end are Montgomery residues all the same (a step domain's sweeps convert)
    fr_rec omega, pre, post, scale;
};

// The argument rules both entries share; no device is needed and nothing is launched or written before they hold.
int frfft_check(amdmsm_ctx *ctx, const fr_vtable *f, const void *values, size_t n, const void *omega, const void *pre,
                const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, const void *out, frfft_plan &plan,
                frfft_params &pr, bool need_vectors = true) {
    if (n & (n - 1)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "n = " + std::to_string(n) + " is not a power of two");
    if (n > FR_FFT_MAX_N) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n = " + std::to_string(n) + ": at most 2^28 records");
    if (frfft_make_plan(f, n, tile_log2, plan))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "tile_log2 = " + std::to_string(tile_log2) + ": 0 or " + std::to_string(FR_TILE_MIN) +
                                                 " .. " + std::to_string(FR_TILE_MAX));
    if (n && need_vectors && !values) return fail(ctx, AMDMSM_ERR_BAD_ARG, "values: null pointer");
    if (n && need_vectors && !out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    if (n > 1 && !omega) return fail(ctx, AMDMSM_ERR_BAD_ARG, "omega: null pointer");
    pr.plain = opts && opts->scalars_plain;
    if (n > 1) {
        pr.omega = fr_read(f, omega, pr.plain);
        fr_rec x = pr.omega;
        const fr_rec minus_one = fr_r_minus(f, fr_from_words(f, f->one));   // -1 as a Montgomery residue: r - R
        for (int b = 0; b + 1 < plan.log_n; ++b) x = fr_mul(f, x, x);
        if (!fr_same(f, x, minus_one))
            return fail(ctx, AMDMSM_ERR_BAD_ARG, "omega is not a primitive n-th root of unity: omega^(n/2) != r - 1 (n = 2^" +
                                                     std::to_string(plan.log_n) + ", 2-adicity of r - 1: " + std::to_string(f->two_adicity) + ")");
    }
    pr.has_pre = pre != nullptr && n > 1;
    pr.has_post = post != nullptr && n > 1;
    pr.has_scale = scale != nullptr;
    if (pre) pr.pre = fr_read(f, pre, pr.plain);
    if (post) pr.post = fr_read(f, post, pr.plain);
    pr.scale = scale ? fr_read(f, scale, pr.plain) : fr_from_words(f, f->one);
    return AMDMSM_OK;
}

// the n / 2 powers of omega, from the context's four most recent or built now; the caller records e->ev when it is done
int frfft_twiddles(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, size_t n, const frfft_params &pr, fr_tw_entry *&e) {
    fr_tw_entry *hit = nullptr, *lru = &ctx->fr_tw[0];
    for (auto &t : ctx->fr_tw) {
        if (t.curve == f->curve && t.n == n && memcmp(t.omega, pr.omega.v, (size_t)f->words * 4) == 0) hit = &t;
        if (t.last_use < lru->last_use) lru = &t;
    }
    e = hit ? hit : lru;
    e->last_use = ++ctx->fr_clock;
    if (!e->ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e->ev, hipEventDisableTiming));
    // the build, or the last reader on another stream, comes first
    if (e->curve >= 0) HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev, 0));
    if (hit) return AMDMSM_OK;
    e->curve = -1;   // not a valid entry until the powers are enqueued
    const int rc = ensure_buf(ctx, e->buf, n / 2 * (size_t)f->words * 4);
    if (rc) return rc;
    const std::vector<uint32_t> table = fr_pow_table(f, pr.omega, 0);
    f->powers(st, table.data(), nullptr, 0, n / 2, (uint32_t *)e->buf.p);
    HIP_TRY(ctx, hipGetLastError());
    // behind the build at once: whatever becomes of this call, a later one on another stream waits for the powers
    HIP_TRY(ctx, hipEventRecord(e->ev, st));
    e->curve = f->curve;
    e->n = n;
    memcpy(e->omega, pr.omega.v, sizeof(e->omega));
    return AMDMSM_OK;
}

// the four vectors of powers of pre and post, laid out as frfft_plan has them behind its first vector; tab: where
// off_pre_col lies
struct frfft_tables {
    uint32_t *pre_col, *pre_row, *post_col, *post_row;
};
frfft_tables frfft_build_tables(const fr_vtable *f, hipStream_t st, const frfft_plan &p, const frfft_params &pr, size_t n, char *tab) {
    const frfft_tables tb = {(uint32_t *)tab, (uint32_t *)(tab + (p.off_pre_row - p.off_pre_col)),
                             (uint32_t *)(tab + (p.off_post_col - p.off_pre_col)), (uint32_t *)(tab + (p.off_post_row - p.off_pre_col))};
    if (pr.has_pre) {   // pre^c, c < n >> t_first, and pre^((n >> t_first) k), k < 2^t_first
        f->powers(st, fr_pow_table(f, pr.pre, 0).data(), nullptr, 0, n >> p.t_first, tb.pre_col);
        f->powers(st, fr_pow_table(f, pr.pre, p.log_n - p.t_first).data(), nullptr, 0, (size_t)1 << p.t_first, tb.pre_row);
    }
    if (pr.has_post) {   // post^q, q < n >> t_last, and scale post^((n >> t_last) k), k < 2^t_last
        f->powers(st, fr_pow_table(f, pr.post, 0).data(), nullptr, 0, n >> p.t_last, tb.post_col);
        f->powers(st, fr_pow_table(f, pr.post, p.log_n - p.t_last).data(), pr.scale.v, 0, (size_t)1 << p.t_last, tb.post_row);
    }
    return tb;
}
// pass k of the plan, log_s stages done before it; in and out are the caller's to fill
fr_pass frfft_pass_of(const frfft_plan &p, const frfft_params &pr, const frfft_tables &tb, const fr_tw_entry *tw, int k, int log_s) {
    const bool first = k == 0, last = k == p.passes - 1;
    const int t = last ? p.t_last : p.tile;
    fr_pass a = {};
    a.tw = tw ? (const uint32_t *)tw->buf.p : nullptr;
    a.pre_col = first && pr.has_pre ? tb.pre_col : nullptr;
    a.pre_row = tb.pre_row;
    a.post_col = last && pr.has_post ? tb.post_col : nullptr;
    a.post_row = tb.post_row;
    a.log_n = p.log_n;
    a.log_r = t;
    a.log_s = log_s;
    a.log_c = std::min(FR_LDS_LOG2 - t, p.log_n - t);
    a.in_plain = first && pr.plain && !pr.mont_in;
    a.out_plain = last && pr.plain && !pr.mont_out;
    a.has_scale = last && pr.has_scale && !pr.has_post;
    memcpy(a.scale, pr.scale.v, sizeof(a.scale));
    return a;
}

// The transform on device-resident vectors, n >= 1; ws: frfft_plan's workspace.  Marks the phases of a timed call.
int frfft_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frfft_plan &p, const frfft_params &pr,
              const uint32_t *d_in, uint32_t *d_out, size_t n, char *ws) {
    fr_tw_entry *tw = nullptr;
    if (n > 1) {
        const int rc = frfft_twiddles(ctx, f, st, n, pr, tw);
        if (rc) return rc;
    }
    const frfft_tables tb = frfft_build_tables(f, st, p, pr, n, ws + p.off_pre_col);
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 1);
    // pass k of P reads what pass k - 1 wrote; the last one writes d_out, and no pass reads and writes one vector --
    // except a lone pass, which is one workgroup that loads everything before it stores anything
    uint32_t *w1 = (uint32_t *)ws, *w2 = (uint32_t *)(ws + p.off_w2);
    const bool third = frfft_third(p, d_in == d_out);
    const uint32_t *src = d_in;
    int log_s = 0;
    for (int k = 0; k < p.passes; ++k) {
        const bool last = k == p.passes - 1;
        uint32_t *dst = last ? d_out : ((p.passes - 1 - k) % 2 == 1 ? w1 : (third ? w2 : d_out));
        fr_pass a = frfft_pass_of(p, pr, tb, tw, k, log_s);
        a.in = src;
        a.out = dst;
        f->pass(st, a);
        src = dst;
        log_s += a.log_r;
    }
    HIP_TRY(ctx, hipGetLastError());
    if (tw) HIP_TRY(ctx, hipEventRecord(tw->ev, st));
    return AMDMSM_OK;
}

// ---- the rules for vectors in device memory, for every Fr entry that takes one.  An absent vector (null) keeps them all.
// Device vectors are moved 16 bytes at a time, 8 for the 10-word fields (fp_load / fp_store); align: another unit than
// the field's (a counter).  what: the operands, as the message names them.
int fr_check_aligned(amdmsm_ctx *ctx, const fr_vtable *f, const char *what, std::initializer_list<const void *> ptrs, size_t align = 0) {
    if (!align) align = f->words % 4 ? 8 : 16;
    for (const void *p : ptrs)
        if ((uintptr_t)p & (align - 1))
            return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(what) + ": not aligned to " + std::to_string(align) + " bytes");
    return AMDMSM_OK;
}
bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
// two vectors that share bytes; same_ok: unless they are one vector (a kernel that reads record i before it writes it)
int fr_check_apart(amdmsm_ctx *ctx, const char *na, const void *a, size_t a_bytes, const char *nb, const void *b, size_t b_bytes,
                   bool same_ok = true) {
    if ((same_ok && a == b) || !ranges_overlap(a, a_bytes, b, b_bytes)) return AMDMSM_OK;
    return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(na) + " and " + nb + " overlap" + (same_ok ? " without being the same vector" : ""));
}
// a small result (a total, a counter) that lies inside one of the vectors of `bytes` each
int fr_check_outside(amdmsm_ctx *ctx, const char *what, const void *small, size_t small_bytes, std::initializer_list<const void *> vecs,
                     size_t bytes) {
    for (const void *v : vecs)
        if (ranges_overlap(small, small_bytes, v, bytes)) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(what) + " lies inside a vector");
    return AMDMSM_OK;
}

// ---- the skeleton of a call on Fr vectors.  A device entry stages nothing: staged = 0, no copies; it takes a
// slot of ws_bytes, runs and ends with phase 1 as its last.  A host entry's vectors lie in the first `staged` bytes of the
// slot, each at the 256-byte-aligned offset its fr_copy names, in front of the same workspace: `up` goes up, run(staged
// vectors, workspace) enqueues the kernels on them, mark 2, `down` comes down, and the stream is drained -- so the caller's
// memory is touched by nothing once the call has returned.  A copy whose host pointer is null or that has no bytes is
// left out.  run places mark 1 itself (the FFT's comes behind its power tables).
struct fr_copy {
    const void *host;
    size_t off, bytes;
};
template <class Run>
int fr_call(amdmsm_ctx *ctx, hipStream_t st, size_t staged, size_t ws_bytes, std::initializer_list<fr_copy> up,
            std::initializer_list<fr_copy> down, Run run) {
    ws_slot *sl = nullptr;
    int rc = call_begin(ctx, st, staged + ws_bytes, sl);
    if (rc) return rc;
    char *base = (char *)sl->ws;
    for (const fr_copy &c : up)
        if (c.host && c.bytes) HIP_TRY(ctx, hipMemcpyAsync(base + c.off, c.host, c.bytes, hipMemcpyHostToDevice, st));
    rc = run(base, base + staged);
    if (!staged) return rc ? rc : call_end(ctx, st, *sl, 1);
    if (rc) {
        (void)hipDeviceSynchronize();   // nothing of this call may still read the caller's vectors
        return rc;
    }
    call_mark(ctx, st, 2);
    for (const fr_copy &c : down)
        if (c.host && c.bytes) HIP_TRY(ctx, hipMemcpyAsync((void *)c.host, base + c.off, c.bytes, hipMemcpyDeviceToHost, st));
    rc = call_end(ctx, st, *sl, 2);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return rc;
}

#define FR_ENTER(ctx)                                                 \
    if (!ctx) return AMDMSM_ERR_BAD_ARG;                              \
    std::lock_guard<std::recursive_mutex> lock_(ctx->mu);             \
    dev_guard guard_(ctx->device)

}   // namespace

extern "C" {

int amdmsm_plan_fr_fft(int curve, size_t n, int tile_log2, size_t out[6]) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out || (n & (n - 1))) return AMDMSM_ERR_BAD_ARG;
    if (n > FR_FFT_MAX_N) return AMDMSM_ERR_TOO_LARGE;
    frfft_plan p;
    if (frfft_make_plan(f, n, tile_log2, p)) return AMDMSM_ERR_BAD_ARG;
    out[0] = (size_t)p.tile;
    out[1] = FR_TILE_MIN;
    out[2] = FR_TILE_MAX;
    out[3] = (size_t)p.passes;
    out[4] = n / 2 * (size_t)p.log_n;
    out[5] = p.ws_plain;
    return AMDMSM_OK;
}

int amdmsm_fr_root_of_unity(int curve, int log2_n, void *r_plain_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!r_plain_out || log2_n < 0 || log2_n > f->two_adicity) return AMDMSM_ERR_BAD_ARG;
    fr_rec x = fr_from_words(f, f->root);
    for (int b = f->two_adicity; b > log2_n; --b) x = fr_mul(f, x, x);
    memcpy(r_plain_out, fr_from_mont(f, x).v, (size_t)f->words * 4);
    return AMDMSM_OK;
}

int amdmsm_fr_fft_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t n, const void *omega, const void *pre,
                         const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frfft_plan p;
    frfft_params pr;
    int rc = frfft_check(ctx, f, d_values, n, omega, pre, post, scale, tile_log2, opts, d_out, p, pr);
    if (rc) return rc;
    if (n) rc = fr_check_aligned(ctx, f, "d_values / d_out", {d_values, d_out});
    if (!rc) rc = fr_check_apart(ctx, "d_values", d_values, n * p.rec, "d_out", d_out, n * p.rec);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n) return AMDMSM_OK;
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, frfft_ws_bytes(p, d_values == d_out), {}, {}, [&](char *, char *ws) {
        return frfft_run(ctx, f, st, p, pr, (const uint32_t *)d_values, (uint32_t *)d_out, n, ws);
    });
}

int amdmsm_fr_fft(amdmsm_ctx *ctx, int curve, const void *values, size_t n, const void *omega, const void *pre, const void *post,
                  const void *scale, int tile_log2, const amdmsm_opts *opts, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frfft_plan p;
    frfft_params pr;
    int rc = frfft_check(ctx, f, values, n, omega, pre, post, scale, tile_log2, opts, out, p, pr);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n) return AMDMSM_OK;
    hipStream_t st = ctx->stream;
    // one staged vector; the transform runs in place on it
    return fr_call(ctx, st, p.vec, frfft_ws_bytes(p, true), {{values, 0, n * p.rec}}, {{out, 0, n * p.rec}}, [&](char *vec, char *ws) {
        return frfft_run(ctx, f, st, p, pr, (const uint32_t *)vec, (uint32_t *)vec, n, ws);
    });
}

int amdmsm_fr_powers_device(amdmsm_ctx *ctx, int curve, const void *base, size_t n, const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    if (n && (!base || !d_out)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (n > ((size_t)1 << 32)) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n = " + std::to_string(n) + ": at most 2^32 records");
    if (n && fr_check_aligned(ctx, f, "d_out", {d_out})) return AMDMSM_ERR_BAD_ARG;
    FR_ENTER(ctx);
    if (!n) return AMDMSM_OK;
    const bool plain = opts && opts->scalars_plain;
    f->powers(stream_of(ctx, opts), fr_pow_table(f, fr_read(f, base, plain), 0).data(), nullptr, plain ? 1 : 0, n, (uint32_t *)d_out);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int amdmsm_fr_muladd_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_a, const void *d_b, const void *d_c,
                            const void *k, const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    if (n && (!d_a || !d_b || !d_out)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "null pointer");
    if (n && fr_check_aligned(ctx, f, "d_a / d_b / d_c / d_out", {d_a, d_b, d_c, d_out})) return AMDMSM_ERR_BAD_ARG;
    FR_ENTER(ctx);
    if (!n) return AMDMSM_OK;
    const bool plain = opts && opts->scalars_plain;
    fr_rec kk;
    if (k) kk = fr_read(f, k, plain);
    f->muladd(stream_of(ctx, opts), n, (const uint32_t *)d_a, (const uint32_t *)d_b, (const uint32_t *)d_c, k ? kk.v : nullptr,
              plain ? 1 : 0, (uint32_t *)d_out);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

}  // extern "C"

// ---- batched transforms: `batch` vectors of one size and one set of parameters through one chain of passes ----
namespace {

// The plan of one vector and what the batch adds: a set is `batch` packed vectors of n records; the workspace is one set,
// one copy of the tables of powers, and the second set that an in-place call of an odd number of passes above one needs.
struct frfft_batch_plan {
    frfft_plan p;
    size_t batch = 0, set = 0, off_tab = 0, off_w2 = 0, ws_plain = 0, ws_all = 0, groups = 0;
    int log_v = 0, log_tiles = 0;   // vectors of a workgroup below 2^10 records, tiles of a vector from there on (log2)
};
void frfft_make_batch_plan(const frfft_plan &p, size_t n, size_t batch, frfft_batch_plan &b) {
    b.p = p;
    b.batch = batch;
    b.set = align_up(std::max<size_t>(1, batch * n) * p.rec, 256);
    b.off_tab = b.set;
    b.off_w2 = b.set + (p.off_w2 - p.off_pre_col);
    b.ws_plain = b.off_w2;
    b.ws_all = b.off_w2 + b.set;
    b.log_v = std::max(0, FR_LDS_LOG2 - p.log_n);
    b.log_tiles = std::max(0, p.log_n - FR_LDS_LOG2);
    b.groups = ((batch + ((size_t)1 << b.log_v) - 1) >> b.log_v) << b.log_tiles;
}
size_t frfft_batch_ws_bytes(const frfft_batch_plan &b, bool in_place) { return frfft_third(b.p, in_place) ? b.ws_all : b.ws_plain; }

// What a batch adds to the rules of one vector of n records (`what`: "n" or "m"): the sizes, the strides (records), and for
// device vectors the ranges [d, d + ((batch - 1) stride + n) rec), which may be one range with one stride or lie apart
int fr_check_batch(amdmsm_ctx *ctx, const fr_vtable *f, const char *what, size_t n, size_t batch, size_t in_stride, size_t out_stride,
                   const void *d_in, const void *d_out, bool device) {
    const size_t rec = (size_t)f->words * 4;
    if (n && batch > FR_FFT_MAX_N / n)
        return fail(ctx, AMDMSM_ERR_TOO_LARGE, "batch = " + std::to_string(batch) + ": batch * " + what + " is at most 2^28 records");
    if (!device || !batch || !n) return AMDMSM_OK;
    const size_t strides[2] = {in_stride, out_stride};
    const char *names[2] = {"in_stride", "out_stride"};
    for (int k = 0; k < 2 && batch > 1; ++k) {
        if (strides[k] > (SIZE_MAX / rec - n) / (batch - 1))
            return fail(ctx, AMDMSM_ERR_TOO_LARGE, std::string(names[k]) + " = " + std::to_string(strides[k]) + ": batch * " + names[k] + " is beyond size_t");
        if (strides[k] < n)
            return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(names[k]) + " = " + std::to_string(strides[k]) + " < " + what + " = " + std::to_string(n) +
                                                     ": the vectors of a batch do not overlap");
    }
    const int rc = fr_check_aligned(ctx, f, "d_values / d_out", {d_in, d_out});
    if (rc) return rc;
    return fr_check_apart(ctx, "d_values", d_in, ((batch - 1) * in_stride + n) * rec, "d_out", d_out, ((batch - 1) * out_stride + n) * rec,
                          batch < 2 || in_stride == out_stride);
}

// frfft_run over a batch: vector v at d_in + v in_stride records and d_out + v out_stride records; the vectors of the
// workspace's sets are packed.  ws: frfft_batch_plan's workspace
int frfft_run_batch(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frfft_batch_plan &b, const frfft_params &pr,
                    const uint32_t *d_in, size_t in_stride, uint32_t *d_out, size_t out_stride, size_t n, char *ws) {
    const frfft_plan &p = b.p;
    fr_tw_entry *tw = nullptr;
    if (n > 1) {
        const int rc = frfft_twiddles(ctx, f, st, n, pr, tw);
        if (rc) return rc;
    }
    const frfft_tables tb = frfft_build_tables(f, st, p, pr, n, ws + b.off_tab);
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 1);
    // the order of the buffers is frfft_run's
    uint32_t *w1 = (uint32_t *)ws, *w2 = (uint32_t *)(ws + b.off_w2);
    const bool third = frfft_third(p, d_in == d_out);
    const uint32_t *src = d_in;
    size_t src_stride = in_stride;
    int log_s = 0;
    for (int k = 0; k < p.passes; ++k) {
        const bool last = k == p.passes - 1;
        uint32_t *dst = last ? d_out : ((p.passes - 1 - k) % 2 == 1 ? w1 : (third ? w2 : d_out));
        fr_pass_batch a = {};
        a.p = frfft_pass_of(p, pr, tb, tw, k, log_s);
        a.p.in = src;
        a.p.out = dst;
        a.in_stride = src_stride;
        a.out_stride = dst == d_out ? out_stride : n;
        a.batch = (uint32_t)b.batch;
        a.log_v = b.log_v;
        a.log_tiles = b.log_tiles;
        f->pass_batch(st, a);
        src = dst;
        src_stride = a.out_stride;
        log_s += a.p.log_r;
    }
    HIP_TRY(ctx, hipGetLastError());
    if (tw) HIP_TRY(ctx, hipEventRecord(tw->ev, st));
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_plan_fr_fft_batch(int curve, size_t n, size_t batch, int tile_log2, size_t out[8]) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out || (n & (n - 1))) return AMDMSM_ERR_BAD_ARG;
    if (n > FR_FFT_MAX_N || (n && batch > FR_FFT_MAX_N / n)) return AMDMSM_ERR_TOO_LARGE;
    frfft_batch_plan b;
    if (frfft_make_plan(f, n, tile_log2, b.p)) return AMDMSM_ERR_BAD_ARG;
    frfft_make_batch_plan(b.p, n, batch, b);
    out[0] = (size_t)b.p.tile;
    out[1] = (size_t)b.p.passes;
    out[2] = (size_t)1 << b.log_v;
    out[3] = n ? b.groups : 0;
    out[4] = n && batch ? (size_t)b.p.passes : 0;
    out[5] = batch * (n / 2 * (size_t)b.p.log_n);
    out[6] = b.ws_plain;
    out[7] = frfft_batch_ws_bytes(b, true);
    return AMDMSM_OK;
}

int amdmsm_fr_fft_batch_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t n, size_t batch, size_t in_stride,
                               size_t out_stride, const void *omega, const void *pre, const void *post, const void *scale, int tile_log2,
                               const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frfft_batch_plan b;
    frfft_params pr;
    int rc = frfft_check(ctx, f, d_values, n, omega, pre, post, scale, tile_log2, opts, d_out, b.p, pr, batch != 0);
    if (!rc) rc = fr_check_batch(ctx, f, "n", n, batch, in_stride, out_stride, d_values, d_out, true);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n || !batch) return AMDMSM_OK;
    frfft_make_batch_plan(b.p, n, batch, b);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, frfft_batch_ws_bytes(b, d_values == d_out), {}, {}, [&](char *, char *ws) {
        return frfft_run_batch(ctx, f, st, b, pr, (const uint32_t *)d_values, in_stride, (uint32_t *)d_out, out_stride, n, ws);
    });
}

int amdmsm_fr_fft_batch(amdmsm_ctx *ctx, int curve, const void *values, size_t n, size_t batch, const void *omega, const void *pre,
                        const void *post, const void *scale, int tile_log2, const amdmsm_opts *opts, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frfft_batch_plan b;
    frfft_params pr;
    int rc = frfft_check(ctx, f, values, n, omega, pre, post, scale, tile_log2, opts, out, b.p, pr, batch != 0);
    if (!rc) rc = fr_check_batch(ctx, f, "n", n, batch, n, n, values, out, false);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n || !batch) return AMDMSM_OK;
    frfft_make_batch_plan(b.p, n, batch, b);
    hipStream_t st = ctx->stream;
    // one staged set of packed vectors; the transforms run in place on it
    const size_t bytes = batch * n * b.p.rec;
    return fr_call(ctx, st, b.set, frfft_batch_ws_bytes(b, true), {{values, 0, bytes}}, {{out, 0, bytes}}, [&](char *set, char *ws) {
        return frfft_run_batch(ctx, f, st, b, pr, (const uint32_t *)set, n, (uint32_t *)set, n, n, ws);
    });
}

}  // extern "C"

// ---- sparse matrix times Fr vector: out[i] = sum_k coeffs[k] x[cols[k]] over the row's entries --------------------------
namespace {

uint32_t frm_env(const char *name) {
    const char *e = getenv(name);
    return e ? (uint32_t)strtoul(e, nullptr, 10) : 0u;
}
bool frm_naive_env() { return env_flag("AMDMSM_FR_MATRIX_NAIVE"); }

bool fr_below_modulus(const fr_vtable *f, const uint32_t *w) {
    for (int j = f->words - 1; j >= 0; --j)
        if (w[j] != f->modulus[j]) return w[j] < f->modulus[j];
    return false;
}

// What plan and load share: the argument rules and the layout.  Nothing is allocated on the device before it returns 0.
// tr: the layout is that of the transpose, which is left there; the rules and what they name are those of M as given.
int frm_prepare(amdmsm_ctx *ctx, const fr_vtable *f, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
                const void *coeffs, int coeffs_plain, frm_layout &L, frm_transposed *tr = nullptr) {
    std::string err;
    const int bad = frm_validate(n_rows, n_cols, offsets, cols, coeffs != nullptr, err);
    if (bad) return fail(ctx, bad == 2 ? AMDMSM_ERR_TOO_LARGE : AMDMSM_ERR_BAD_ARG, err);
    if (tr) frm_transpose(n_rows, n_cols, offsets, cols, *tr);
    // 1 and r - 1 in the form the coefficients come in
    const fr_rec one = coeffs_plain ? fr_small(1) : fr_from_words(f, f->one), minus_one = fr_r_minus(f, one), zero;
    const size_t rec = (size_t)f->words * 4;
    uint64_t bad_entry = 0;
    const auto cls_of = [&](uint64_t k) -> uint32_t {
        uint32_t w[FR_MAX_WORDS];
        memcpy(w, (const char *)coeffs + k * rec, rec);   // the caller's array needs no alignment
        if (!fr_below_modulus(f, w)) return FRM_BAD;
        if (!memcmp(w, one.v, rec)) return FRM_PLUS;
        if (!memcmp(w, minus_one.v, rec)) return FRM_MINUS;
        if (!memcmp(w, zero.v, rec)) return FRM_ZERO;
        return FRM_GEN;
    };
    const uint32_t want_wave = frm_env("AMDMSM_FR_MATRIX_WAVE_ROW"), want_split = frm_env("AMDMSM_FR_MATRIX_SPLIT_ROW");
    bool ok;
    if (tr) {
        ok = frm_build(n_cols, tr->offsets.data(), tr->rows.data(), [&](uint64_t k) { return cls_of(tr->src[k]); }, want_wave,
                       want_split, L, bad_entry);
        // the entry a plain load would have named: the first in M's order
        for (uint64_t k = 0; !ok && k < L.nnz; ++k)
            if (cls_of(k) == FRM_BAD) {
                bad_entry = k;
                break;
            }
    } else {
        ok = frm_build(n_rows, offsets, cols, cls_of, want_wave, want_split, L, bad_entry);
    }
    if (!ok) return fail(ctx, AMDMSM_ERR_BAD_ARG, "entry " + std::to_string(bad_entry) + ": coefficient >= r");
    return AMDMSM_OK;
}

size_t frm_device_bytes(const fr_vtable *f, const frm_layout &L, size_t n_rows, bool naive) {
    const size_t rec = (size_t)f->words * 4;
    if (naive) return (n_rows + 1) * 8 + L.nnz * 4 + L.nnz * rec;
    return L.words.size() * 4 + L.gen_src.size() * rec + L.desc.size() * sizeof(frm_desc) + L.lane_rows.size() * 4 +
           L.comb.size() * sizeof(frm_comb);
}

std::atomic<uint64_t> g_fr_matrix_id{1};   // ids are never reused, in any context: a stale or foreign handle finds nothing

fr_matrix *frm_find(amdmsm_ctx *ctx, uint64_t id) {
    for (fr_matrix *m : ctx->fr_mats)
        if (m->id == id) return m;
    return nullptr;
}

int frm_upload(amdmsm_ctx *ctx, void *&d, const void *h, size_t bytes) {
    if (!bytes) return AMDMSM_OK;
    HIP_TRY(ctx, hipMalloc(&d, bytes));
    HIP_TRY(ctx, hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return AMDMSM_OK;
}

void frm_release(fr_matrix *m) {
    for (void *p : {m->words, m->coef, m->desc, m->lane_rows, m->comb, m->offsets, m->cols})
        if (p) (void)hipFree(p);
    for (auto &u : m->users) (void)hipEventDestroy(u.second);
    delete m;
}

// The argument rules of both apply entries, the handle found; device: the vectors are HBM addresses
int frm_check_apply(amdmsm_ctx *ctx, uint64_t mat, const void *x, size_t n_x, const void *out, size_t n_out, bool device,
                    fr_matrix *&m, const fr_vtable *&f) {
    m = frm_find(ctx, mat);
    if (!m) return fail(ctx, AMDMSM_ERR_BAD_ARG, "matrix handle " + std::to_string(mat) + ": not a live handle of this context");
    f = find_frvt(m->curve);
    if (n_x < m->n_cols)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "n_x = " + std::to_string(n_x) + " < n_cols = " + std::to_string(m->n_cols));
    if (n_out < m->n_rows)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "n_out = " + std::to_string(n_out) + " < n_rows = " + std::to_string(m->n_rows));
    if (n_x > FRM_MAX_DIM || n_out > FRM_MAX_DIM)
        return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n_x / n_out: at most 2^28 records");
    if (n_out && !out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    if (m->kept && !x) return fail(ctx, AMDMSM_ERR_BAD_ARG, "x: null pointer");
    if (!device) return AMDMSM_OK;
    const size_t rec = (size_t)f->words * 4;
    const int rc = fr_check_aligned(ctx, f, "d_x / d_out", {x, out});
    // stricter than the other entries: a row reads any column, so d_x == d_out is refused too
    return rc ? rc : fr_check_apart(ctx, "d_x", x, n_x * rec, "d_out", out, n_out * rec, false);
}

// the workspace of an apply: the partial sums
size_t frm_ws_bytes(const fr_vtable *f, const fr_matrix *m) { return align_up(((size_t)m->n_partials + 1) * f->words * 4, 256); }

int frm_record_user(amdmsm_ctx *ctx, hipStream_t st, fr_matrix *m);

// the kernels of one apply on device vectors, behind mark 1; partial: room for n_partials records
int frm_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, fr_matrix *m, const uint32_t *d_x, uint32_t *d_out, size_t n_out,
            uint32_t *partial) {
    call_mark(ctx, st, 1);
    if (m->naive) {
        f->matrix_naive(st, m->n_rows, n_out, (const uint64_t *)m->offsets, (const uint32_t *)m->cols, (const uint32_t *)m->coef, d_x,
                        d_out);
    } else {
        frm_args a = {};
        a.words = (const uint32_t *)m->words;
        a.coef = (const uint32_t *)m->coef;
        a.desc = (const frm_desc *)m->desc;
        a.lane_rows = (const uint32_t *)m->lane_rows;
        a.comb = (const frm_comb *)m->comb;
        a.x = d_x;
        a.out = d_out;
        a.partial = partial;
        a.n_desc = m->n_desc;
        a.n_comb = m->n_comb;
        a.n_rows = m->n_rows;
        a.n_out = n_out;
        f->matrix_apply(st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return frm_record_user(ctx, st, m);
}

// behind this user of the handle: what amdmsm_fr_matrix_free waits for
int frm_record_user(amdmsm_ctx *ctx, hipStream_t st, fr_matrix *m) {
    hipEvent_t *ev = nullptr;
    for (auto &u : m->users)
        if (u.first == st) ev = &u.second;
    if (!ev) {
        hipEvent_t e = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m->users.emplace_back(st, e);
        ev = &m->users.back().second;
    }
    HIP_TRY(ctx, hipEventRecord(*ev, st));
    return AMDMSM_OK;
}

// plan and load of a matrix or, with `transposed`, of its transpose: the handle then has n_cols rows and n_rows columns
int frm_plan(int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols, const void *coeffs,
             int coeffs_plain, bool transposed, size_t *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out) return AMDMSM_ERR_BAD_ARG;
    frm_layout L;
    frm_transposed tr;
    const int rc = frm_prepare(nullptr, f, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, L, transposed ? &tr : nullptr);
    if (rc) return rc;
    const bool naive = frm_naive_env();
    out[0] = L.nnz;
    out[1] = L.cnt[FRM_GEN];
    out[2] = L.cnt[FRM_PLUS];
    out[3] = L.cnt[FRM_MINUS];
    out[4] = L.cnt[FRM_ZERO];
    out[5] = L.rows_lane;
    out[6] = L.rows_wave;
    out[7] = L.rows_split;
    out[8] = L.t_wave;
    out[9] = L.t_split;
    out[10] = L.longest;
    out[11] = frm_device_bytes(f, L, transposed ? n_cols : n_rows, naive);
    out[12] = naive ? 1 : 1 + (L.comb.empty() ? 0 : 1);
    out[13] = f->matrix_chunk;
    out[14] = L.desc.size();
    out[15] = L.n_partials;
    return AMDMSM_OK;
}

int frm_load(amdmsm_ctx *ctx, int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
             const void *coeffs, int coeffs_plain, bool transposed, uint64_t *mat) {
    if (mat) *mat = 0;   // no handle is ever 0
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    if (!mat) return fail(ctx, AMDMSM_ERR_BAD_ARG, "mat: null pointer");
    frm_layout L;
    frm_transposed tr;
    int rc = frm_prepare(ctx, f, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, L, transposed ? &tr : nullptr);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (transposed) {   // from here on the matrix is the transpose
        std::swap(n_rows, n_cols);
        offsets = tr.offsets.data();
        cols = tr.rows.data();
    }
    const size_t rec = (size_t)f->words * 4, N = (size_t)f->words;
    const fr_rec r2 = fr_from_words(f, f->r2);
    const auto mont = [&](uint64_t k, uint32_t *dst) {   // coefficient k of the matrix as a Montgomery residue
        fr_rec c;
        memcpy(c.v, (const char *)coeffs + (transposed ? tr.src[k] : k) * rec, rec);
        if (coeffs_plain) c = fr_mul(f, c, r2);
        memcpy(dst, c.v, rec);
    };
    fr_matrix *m = new fr_matrix();
    m->curve = curve;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->naive = frm_naive_env();
    std::vector<uint32_t> coef;
    if (m->naive) {
        m->kept = L.nnz;
        coef.resize(L.nnz * N);
        for (uint64_t k = 0; k < L.nnz; ++k) mont(k, &coef[k * N]);
        const uint64_t none[1] = {0};
        rc = frm_upload(ctx, m->offsets, n_rows ? offsets : none, (n_rows + 1) * 8);
        if (!rc) rc = frm_upload(ctx, m->cols, cols, L.nnz * 4);
    } else {
        m->kept = L.nnz - L.cnt[FRM_ZERO];
        coef.resize(L.gen_src.size() * N);
        for (size_t g = 0; g < L.gen_src.size(); ++g) mont(L.gen_src[g], &coef[g * N]);
        m->n_desc = (uint32_t)L.desc.size();
        m->n_comb = (uint32_t)L.comb.size();
        m->n_partials = L.n_partials;
        m->job_gen.reserve(L.desc.size() + 1);
        for (const frm_desc &d : L.desc) m->job_gen.push_back(d.gen_base);
        m->job_gen.push_back((uint32_t)L.gen_src.size());
        rc = frm_upload(ctx, m->words, L.words.data(), L.words.size() * 4);
        if (!rc) rc = frm_upload(ctx, m->desc, L.desc.data(), L.desc.size() * sizeof(frm_desc));
        if (!rc) rc = frm_upload(ctx, m->lane_rows, L.lane_rows.data(), L.lane_rows.size() * 4);
        if (!rc) rc = frm_upload(ctx, m->comb, L.comb.data(), L.comb.size() * sizeof(frm_comb));
    }
    if (!rc) rc = frm_upload(ctx, m->coef, coef.data(), coef.size() * 4);
    if (rc) {
        frm_release(m);
        return rc;
    }
    m->id = g_fr_matrix_id.fetch_add(1);
    ctx->fr_mats.push_back(m);
    *mat = m->id;
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_plan_fr_matrix(int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols, const void *coeffs,
                          int coeffs_plain, size_t out[AMDMSM_FR_MATRIX_PLAN_WORDS]) {
    return frm_plan(curve, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, false, out);
}
int amdmsm_plan_fr_matrix_transposed(int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
                                     const void *coeffs, int coeffs_plain, size_t out[AMDMSM_FR_MATRIX_PLAN_WORDS]) {
    return frm_plan(curve, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, true, out);
}

int amdmsm_fr_matrix_load(amdmsm_ctx *ctx, int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols,
                          const void *coeffs, int coeffs_plain, uint64_t *mat) {
    return frm_load(ctx, curve, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, false, mat);
}
int amdmsm_fr_matrix_load_transposed(amdmsm_ctx *ctx, int curve, size_t n_rows, size_t n_cols, const uint64_t *offsets,
                                     const uint32_t *cols, const void *coeffs, int coeffs_plain, uint64_t *mat) {
    return frm_load(ctx, curve, n_rows, n_cols, offsets, cols, coeffs, coeffs_plain, true, mat);
}

int amdmsm_fr_matrix_free(amdmsm_ctx *ctx, uint64_t mat) {
    FR_ENTER(ctx);
    fr_matrix *m = frm_find(ctx, mat);
    if (!m) return fail(ctx, AMDMSM_ERR_BAD_ARG, "matrix handle " + std::to_string(mat) + ": not a live handle of this context");
    for (auto &u : m->users) (void)hipEventSynchronize(u.second);   // the applies that still read the arrays
    ctx->fr_mats.erase(std::find(ctx->fr_mats.begin(), ctx->fr_mats.end(), m));
    frm_release(m);
    return AMDMSM_OK;
}

int amdmsm_fr_matrix_apply_device(amdmsm_ctx *ctx, uint64_t mat, const void *d_x, size_t n_x, void *d_out, size_t n_out,
                                  const amdmsm_opts *opts) {
    CHECK_OPTS(ctx, opts);
    FR_ENTER(ctx);
    fr_matrix *m = nullptr;
    const fr_vtable *f = nullptr;
    int rc = frm_check_apply(ctx, mat, d_x, n_x, d_out, n_out, true, m, f);
    if (rc) return rc;
    if (!n_out) return AMDMSM_OK;
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, frm_ws_bytes(f, m), {}, {}, [&](char *, char *ws) {
        return frm_run(ctx, f, st, m, (const uint32_t *)d_x, (uint32_t *)d_out, n_out, (uint32_t *)ws);
    });
}

int amdmsm_fr_matrix_apply(amdmsm_ctx *ctx, uint64_t mat, const void *x, size_t n_x, void *out, size_t n_out,
                           const amdmsm_opts *opts) {
    CHECK_OPTS(ctx, opts);
    FR_ENTER(ctx);
    fr_matrix *m = nullptr;
    const fr_vtable *f = nullptr;
    int rc = frm_check_apply(ctx, mat, x, n_x, out, n_out, false, m, f);
    if (rc) return rc;
    if (!n_out) return AMDMSM_OK;
    hipStream_t st = ctx->stream;
    const size_t rec = (size_t)f->words * 4;
    // staged: the vector and the result, in that order
    const size_t x_bytes = align_up((n_x ? n_x : 1) * rec, 256), out_bytes = align_up(n_out * rec, 256);
    return fr_call(ctx, st, x_bytes + out_bytes, frm_ws_bytes(f, m), {{x, 0, n_x * rec}}, {{out, x_bytes, n_out * rec}},
                   [&](char *vecs, char *ws) {
                       return frm_run(ctx, f, st, m, (const uint32_t *)vecs, (uint32_t *)(vecs + x_bytes), n_out, (uint32_t *)ws);
                   });
}

}  // extern "C"

// ---- sparse matrix times point vector: out[i] = sum_k coeff[k] P[col[k]] over the kept entries of row i --------------------
namespace {

// The wave jobs of the handle are worked through in chunks [job0, job1): first the general entries of the chunk --
// gm_gather, smv_table, smv_ladder with the handle's coefficients, import_bases in normal form -- then gm_apply over
// the same jobs.  rank0, cnt: the chunk's general entries in the handle's side array.
struct gm_chunk {
    uint32_t job0, job1, rank0, cnt;
};
// Workspace of the call's slot: gathered points (the products as compact affine records once the table is built) |
// table and its scratch | products as libff records | partial sums.  The normalisation of an AMDMSM_OUT_AFFINE output
// runs behind everything else and takes its n_rows compact affine records from the start of the slot.
struct gm_plan {
    std::vector<gm_chunk> chunks;
    size_t cn = 0;   // the most general entries of a chunk
    size_t off_table = 0, off_tmp = 0, off_prod = 0, off_part = 0, ws_bytes = 0, launches = 0;
};
gm_plan gm_make_plan(const group_vtable *vt, const fr_matrix *m, size_t chunk_entries) {
    gm_plan p;
    const size_t aff = (size_t)vt->el_words * 8, xyz = (size_t)vt->el_words * 12, zz = (size_t)vt->el_words * 16;
    const size_t part = align_up(((size_t)m->n_partials + 1) * zz, 256);
    const size_t per = aff + 2 * smv_table_bytes(vt, 1) + xyz, n_gen = m->job_gen.empty() ? 0 : m->job_gen.back();
    const size_t want = vec_chunk_points(per, part < SMV_WS_BUDGET / 2 ? part : SMV_WS_BUDGET / 2, n_gen ? n_gen : 1, chunk_entries);
    for (uint32_t j = 0; j < m->n_desc;) {
        gm_chunk c = {j, j + 1, m->job_gen[j], 0};
        while (c.job1 < m->n_desc && (size_t)m->job_gen[c.job1 + 1] - c.rank0 <= want) ++c.job1;   // a job is never split
        c.cnt = m->job_gen[c.job1] - c.rank0;
        if (c.cnt > p.cn) p.cn = c.cnt;
        p.launches += c.cnt ? 5 : 1;
        p.chunks.push_back(c);
        j = c.job1;
    }
    if (m->n_comb) ++p.launches;
    p.off_table = align_up(p.cn * aff, 256);
    p.off_tmp = p.off_table + align_up(smv_table_bytes(vt, p.cn), 256);
    p.off_prod = p.off_tmp + align_up(smv_table_bytes(vt, p.cn), 256);
    p.off_part = p.off_prod + align_up(p.cn * xyz, 256);
    p.ws_bytes = std::max(p.off_part + part, align_up(m->n_rows * aff, 256));
    return p;
}

// The argument rules of the three entries up to the handle, in the order the header gives; the caller has refused an
// unknown group already.
int gm_check_handle(amdmsm_ctx *ctx, int curve, uint64_t mat, fr_matrix *&m) {
    m = frm_find(ctx, mat);
    if (!m) return fail(ctx, AMDMSM_ERR_BAD_ARG, "mat: handle " + std::to_string(mat) + " is not a live handle of this context");
    if (m->curve != curve)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "mat: handle " + std::to_string(mat) + " belongs to curve " + std::to_string(m->curve) +
                                                 ", not " + std::to_string(curve));
    if (m->naive) return fail(ctx, AMDMSM_ERR_BAD_ARG, "mat: handle " + std::to_string(mat) + " was loaded under AMDMSM_FR_MATRIX_NAIVE and has no resident form");
    return AMDMSM_OK;
}
// ... and of both apply entries behind it.  device: points and out are HBM addresses, compact affine records in and
// packed libff records out; else host vectors, the points stride_bytes apart.
int gm_check(amdmsm_ctx *ctx, const group_vtable *vt, int curve, uint64_t mat, const void *points, size_t n_points, const void *out,
             bool device, size_t &stride_bytes, fr_matrix *&m) {
    int rc = gm_check_handle(ctx, curve, mat, m);
    if (rc) return rc;
    if (n_points < m->n_cols)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "n_points = " + std::to_string(n_points) + " < n_cols = " + std::to_string(m->n_cols));
    if (m->n_rows && !out) return fail(ctx, AMDMSM_ERR_BAD_ARG, device ? "d_out_xyz: null pointer" : "out_xyz: null pointer");
    if (m->n_rows && m->kept && !points)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, device ? "d_points_affine: null pointer" : "points_xyz: null pointer");
    const size_t aff = (size_t)vt->el_words * 8, xyz = (size_t)vt->el_words * 12;
    if (device) {
        rc = dev_check_aligned(ctx, "d_points_affine", points, rec_align(vt));
        if (!rc) rc = dev_check_aligned(ctx, "d_out_xyz", out, rec_align(vt));
        if (!rc) rc = fr_check_apart(ctx, "d_points_affine", points, n_points * aff, "d_out_xyz", out, m->n_rows * xyz, false);
    } else {
        rc = vec_check_stride(ctx, vt, stride_bytes, "stride_bytes: not a stride of libff records");
        if (!rc && n_points)
            rc = fr_check_apart(ctx, "points_xyz", points, (n_points - 1) * stride_bytes + xyz, "out_xyz", out, m->n_rows * xyz, false);
    }
    if (rc) return rc;
    if (n_points > FRM_MAX_DIM) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n_points = " + std::to_string(n_points) + ": at most 2^28 points");
    return AMDMSM_OK;
}

// the kernels of one apply on device-resident points, between the call's first mark and its last; n_rows > 0
int gm_run(amdmsm_ctx *ctx, const group_vtable *vt, hipStream_t st, fr_matrix *m, const gm_plan &p, const uint32_t *d_points,
           uint32_t *d_out, const vec_opts &vo, char *ws) {
    gm_args a = {};
    a.words = (const uint32_t *)m->words;
    a.desc = (const frm_desc *)m->desc;
    a.lane_rows = (const uint32_t *)m->lane_rows;
    a.points = d_points;
    a.prod = (uint32_t *)ws;
    a.out = d_out;
    a.partial = (uint32_t *)(ws + p.off_part);
    a.form = vo.kernel_form;
    uint32_t *table = (uint32_t *)(ws + p.off_table), *tmp = (uint32_t *)(ws + p.off_tmp), *prod_xyz = (uint32_t *)(ws + p.off_prod);
    for (const gm_chunk &c : p.chunks) {
        a.job0 = c.job0;
        a.n_jobs = c.job1 - c.job0;
        a.first_rank = c.rank0;
        if (c.cnt) {
            call_mark(ctx, st, 1);
            vt->gm_gather(st, a);
            vt->smv_table(st, a.prod, c.cnt, tmp, table);
            vt->smv_ladder(st, table, c.cnt, (const uint32_t *)m->coef + (size_t)c.rank0 * vt->fr_words, 1, AMDMSM_OUT_LIBFF, prod_xyz);
            // the gathered points are dead behind the table: the products take their place, the group's zero as (0, 0)
            vt->import_bases(st, prod_xyz, (size_t)vt->el_words * 3, 0, c.cnt, a.prod);
        }
        call_mark(ctx, st, 2);
        vt->gm_apply(st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    vt->gm_combine(st, (const frm_comb *)m->comb, m->n_comb, a.partial, a.form, d_out);
    call_mark(ctx, st, 3);
    vec_finish(vt, st, vo, d_out, m->n_rows, (uint32_t *)ws);
    HIP_TRY(ctx, hipGetLastError());
    return frm_record_user(ctx, st, m);
}

int gm_check_form(amdmsm_ctx *ctx, const vec_opts &vo) {
    if (vo.form != AMDMSM_OUT_LIBFF && vo.form != AMDMSM_OUT_AFFINE)
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "opts->out_form: AMDMSM_OUT_LIBFF or AMDMSM_OUT_AFFINE");
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

#define GM_ENTER(ctx, curve, group)                                                \
    SMV_REFUSE_UNKNOWN(ctx, curve, group);                                         \
    if (!ctx) return fail(ctx, AMDMSM_ERR_BAD_ARG, "ctx: null pointer");           \
    GET_VT(ctx, curve, group)

int amdmsm_plan_group_matrix(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, size_t chunk_entries, size_t out[8]) {
    GM_ENTER(ctx, curve, group);
    fr_matrix *m = nullptr;
    const int rc = gm_check_handle(ctx, curve, mat, m);
    if (rc) return rc;
    if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "out: null pointer");
    const gm_plan p = gm_make_plan(vt, m, chunk_entries);
    const size_t n_gen = m->job_gen.empty() ? 0 : m->job_gen.back();
    out[0] = n_gen;
    out[1] = m->kept - n_gen;
    out[2] = m->n_desc;
    out[3] = m->n_partials;
    out[4] = p.chunks.size();
    out[5] = p.ws_bytes;
    out[6] = p.launches;
    out[7] = 0;
    return AMDMSM_OK;
}

int amdmsm_group_matrix_apply_device(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, const void *d_points_affine,
                                     size_t n_points, void *d_out_xyz, size_t chunk_entries, const amdmsm_opts *opts) {
    GM_ENTER(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    int rc = gm_check_form(ctx, vo);
    if (rc) return rc;
    fr_matrix *m = nullptr;
    size_t stride = 0;
    rc = gm_check(ctx, vt, curve, mat, d_points_affine, n_points, d_out_xyz, true, stride, m);
    if (rc || !m->n_rows) return rc;
    hipStream_t st = stream_of(ctx, opts);
    const gm_plan p = gm_make_plan(vt, m, chunk_entries);
    ws_slot *sl = nullptr;
    rc = call_begin(ctx, st, p.ws_bytes, sl);
    if (rc) return rc;
    rc = gm_run(ctx, vt, st, m, p, (const uint32_t *)d_points_affine, (uint32_t *)d_out_xyz, vo, (char *)sl->ws);
    if (rc) return rc;
    return call_end(ctx, st, *sl);
}

int amdmsm_group_matrix_apply(amdmsm_ctx *ctx, int curve, int group, uint64_t mat, const void *points_xyz, size_t stride_bytes,
                              int base_form, size_t n_points, void *out_xyz, size_t chunk_entries, const amdmsm_opts *opts) {
    GM_ENTER(ctx, curve, group);
    CHECK_OPTS(ctx, opts);
    const vec_opts vo = vec_opts_of(opts);
    int rc = gm_check_form(ctx, vo);
    if (rc) return rc;
    fr_matrix *m = nullptr;
    rc = gm_check(ctx, vt, curve, mat, points_xyz, n_points, out_xyz, false, stride_bytes, m);
    if (rc || !m->n_rows) return rc;
    hipStream_t st = ctx->stream;
    const size_t xyz_bytes = (size_t)vt->el_words * 12, aff_bytes = (size_t)vt->el_words * 8;
    const size_t n_up = points_xyz ? n_points : 0;   // a matrix without kept entries reads no point
    const gm_plan p = gm_make_plan(vt, m, chunk_entries);
    rc = ensure_buf(ctx, ctx->hb_src, n_up * stride_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->hb_aff, n_up * aff_bytes);
    if (rc == AMDMSM_OK) rc = ensure_buf(ctx, ctx->fb.out, m->n_rows * xyz_bytes);
    ws_slot *sl = nullptr;
    if (rc == AMDMSM_OK) rc = call_begin(ctx, st, p.ws_bytes, sl);
    if (rc) return rc;
    if (n_up) rc = vec_upload(ctx, vt, st, points_xyz, stride_bytes, base_form, 0, n_up, ctx->hb_aff.p);
    if (!rc) rc = gm_run(ctx, vt, st, m, p, (const uint32_t *)ctx->hb_aff.p, (uint32_t *)ctx->fb.out.p, vo, (char *)sl->ws);
    if (rc) {
        (void)hipDeviceSynchronize();   // nothing of this call may still touch the staging buffers
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, ctx->fb.out.p, m->n_rows * xyz_bytes, hipMemcpyDeviceToHost, st));
    rc = call_end(ctx, st, *sl);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return rc;
}

}  // extern "C"

// ---- scans and batch inversion over Fr vectors: y_i = a_i y_(i-1) + b_i, out[i] = 1 / in[i] -------------------------------
namespace {

constexpr int FRS_KIND_MASK = AMDMSM_SCAN_KIND_A | AMDMSM_SCAN_KIND_B | AMDMSM_SCAN_KIND_INVERT;
constexpr int FRS_FLAG_MASK = AMDMSM_SCAN_REVERSE | AMDMSM_SCAN_EXCLUSIVE;

bool frs_naive_env() { return env_flag("AMDMSM_FR_SCAN_NAIVE"); }

// x^(r - 2) for a Montgomery residue x: one Fermat power, r - 2 scanned from its top bit
fr_rec fr_inv_host(const fr_vtable *f, const fr_rec &x) {
    const fr_rec e = fr_r_minus(f, fr_small(2));
    fr_rec acc = fr_from_words(f, f->one);
    for (int i = f->words * 32 - 1; i >= 0; --i) {
        acc = fr_mul(f, acc, acc);
        if ((e.v[i >> 5] >> (i & 31)) & 1u) acc = fr_mul(f, acc, x);
    }
    return acc;
}

// what a call runs with: the layout, and the host records as Montgomery residues
struct frs_call {
    frs_layout L;
    bool plain = false, naive = false, invert = false;
    int has_a = 0, has_b = 0, flags = 0;
    fr_rec a_const, init;
    size_t rec = 0;
};

// The argument rules of the four entries; nothing is launched or written and the context is not looked at before they
// hold.  device: the vectors are HBM addresses (alignment, overlap).  vec_a: d_a / d_values; total: d_total / d_zero_count
int frs_check(amdmsm_ctx *ctx, const fr_vtable *f, size_t n, const void *vec_a, const void *a_const, const void *vec_b,
              const void *init, int flags, int tile_log2, const amdmsm_opts *opts, const void *out, const void *total, bool invert,
              bool device, frs_call &c) {
    c.rec = (size_t)f->words * 4;
    c.plain = opts && opts->scalars_plain;
    c.naive = frs_naive_env();
    c.invert = invert;
    c.flags = flags;
    if (n > FRS_MAX_N) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n = " + std::to_string(n) + ": at most 2^28 records");
    if (flags & ~FRS_FLAG_MASK) return fail(ctx, AMDMSM_ERR_BAD_ARG, "flags = " + std::to_string(flags) + ": unknown bits");
    const char *na = invert ? "values" : "a", *no = "out";
    if (!invert) {
        if (vec_a && a_const) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a and a_const: both given");
        if (!vec_a && !a_const && !vec_b) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a and b: both absent");
    }
    c.has_a = vec_a ? 1 : (a_const ? 2 : 0);
    c.has_b = vec_b ? 1 : 0;
    if (n) {
        if (invert && !vec_a) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(na) + ": null pointer");
        if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(no) + ": null pointer");
    }
    if (device) {
        const char *da = invert ? "d_values" : "d_a", *dt = invert ? "d_zero_count" : "d_total";
        const size_t bytes = n * c.rec;
        int rc = AMDMSM_OK;
        if (n) rc = fr_check_aligned(ctx, f, da, {vec_a});
        if (n && !rc) rc = fr_check_aligned(ctx, f, "d_b", {vec_b});
        if (n && !rc) rc = fr_check_aligned(ctx, f, "d_out", {out});
        if (!rc) rc = fr_check_aligned(ctx, f, dt, {total}, invert ? 8 : 0);
        if (!rc) rc = fr_check_apart(ctx, da, vec_a, bytes, "d_out", out, bytes);
        if (!rc) rc = fr_check_apart(ctx, "d_b", vec_b, bytes, "d_out", out, bytes);
        if (!rc) rc = fr_check_outside(ctx, dt, total, invert ? 8 : c.rec, {vec_a, vec_b, out}, bytes);
        if (rc) return rc;
    }
    if (!frs_make_layout(n, tile_log2, c.rec, invert, c.naive, c.L))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "tile_log2 = " + std::to_string(tile_log2) + ": 0 or " + std::to_string(FRS_TILE_MIN) +
                                                 " .. " + std::to_string(FRS_TILE_MAX));
    if (a_const && !fr_below_modulus(f, (const uint32_t *)a_const)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "a_const: not below r");
    if (init && !fr_below_modulus(f, (const uint32_t *)init)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "init: not below r");
    if (a_const) c.a_const = fr_read(f, a_const, c.plain);
    if (init) c.init = fr_read(f, init, c.plain);
    else if (!c.has_b) c.init = fr_from_words(f, f->one);
    return AMDMSM_OK;
}

// the launches of one call on device vectors, behind mark 1; ws: the layout's workspace
int frs_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frs_call &c, size_t n, const void *d_a, const void *d_b,
            void *d_out, void *d_total, char *ws) {
    call_mark(ctx, st, 1);
    frs_args a = {};
    a.a = (const uint32_t *)d_a;
    a.b = (const uint32_t *)d_b;
    a.out = (uint32_t *)d_out;
    if (c.invert) a.zero_count = (uint64_t *)d_total;
    else a.total = (uint32_t *)d_total;
    a.ws_a = (uint32_t *)(ws + c.L.off_a);
    a.ws_b = (uint32_t *)(ws + c.L.off_b);
    a.ws_in = (uint32_t *)(ws + c.L.off_in);
    a.ws_cnt = (uint32_t *)(ws + c.L.off_cnt);
    a.n = n;
    a.tiles = (uint32_t)c.L.tiles;
    a.tile_log2 = c.L.tile_log2;
    a.has_a = c.invert ? 1 : c.has_a;
    a.has_b = c.has_b;
    a.reverse = (c.flags & AMDMSM_SCAN_REVERSE) ? 1 : 0;
    a.exclusive = (c.flags & AMDMSM_SCAN_EXCLUSIVE) ? 1 : 0;
    a.plain = c.plain ? 1 : 0;
    a.invert = c.invert ? 1 : 0;
    memcpy(a.a_const, c.a_const.v, sizeof(a.a_const));
    memcpy(a.init, c.init.v, sizeof(a.init));
    if (c.naive) f->scan_naive(st, a);
    else f->scan(st, a);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

int frs_device_entry(amdmsm_ctx *ctx, int curve, size_t n, const void *d_a, const void *a_const, const void *d_b, const void *init,
                     int flags, int tile_log2, const amdmsm_opts *opts, void *d_out, void *d_total, bool invert) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frs_call c;
    int rc = frs_check(ctx, f, n, d_a, a_const, d_b, init, flags, tile_log2, opts, d_out, d_total, invert, true, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n && !d_total) return AMDMSM_OK;
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, c.L.ws_bytes, {}, {},
                   [&](char *, char *ws) { return frs_run(ctx, f, st, c, n, d_a, d_b, d_out, d_total, ws); });
}

int frs_host_entry(amdmsm_ctx *ctx, int curve, size_t n, const void *a, const void *a_const, const void *b, const void *init,
                   int flags, int tile_log2, const amdmsm_opts *opts, void *out, void *total, bool invert) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frs_call c;
    int rc = frs_check(ctx, f, n, a, a_const, b, init, flags, tile_log2, opts, out, total, invert, false, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!n && !total) return AMDMSM_OK;
    hipStream_t st = ctx->stream;
    // staged: the two vectors and the total (or the zero count), in that order; the result takes the place of the first
    // vector that is given
    const size_t vec = align_up((n ? n : 1) * c.rec, 256), bytes = n * c.rec, off_out = a ? 0 : vec, off_total = 2 * vec;
    return fr_call(ctx, st, 2 * vec + 256, c.L.ws_bytes, {{a, 0, bytes}, {b, vec, bytes}},
                   {{out, off_out, bytes}, {total, off_total, invert ? 8 : c.rec}}, [&](char *vecs, char *ws) {
                       return frs_run(ctx, f, st, c, n, a ? vecs : nullptr, b ? vecs + vec : nullptr, vecs + off_out,
                                      total ? vecs + off_total : nullptr, ws);
                   });
}

}   // namespace

extern "C" {

int amdmsm_fr_inverse(int curve, const void *x, int plain, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!x || !out) return AMDMSM_ERR_BAD_ARG;
    const fr_rec raw = fr_from_words(f, (const uint32_t *)x), zero;
    if (!fr_below_modulus(f, raw.v) || fr_same(f, raw, zero)) return AMDMSM_ERR_BAD_ARG;
    fr_rec r = fr_inv_host(f, fr_read(f, x, plain != 0));
    if (plain) r = fr_from_mont(f, r);
    memcpy(out, r.v, (size_t)f->words * 4);
    return AMDMSM_OK;
}

int amdmsm_plan_fr_scan(int curve, size_t n, int kind_and_flags, int tile_log2, size_t out[8]) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out || (kind_and_flags & ~(FRS_KIND_MASK | FRS_FLAG_MASK))) return AMDMSM_ERR_BAD_ARG;
    const bool invert = (kind_and_flags & AMDMSM_SCAN_KIND_INVERT) != 0;
    const bool ha = (kind_and_flags & AMDMSM_SCAN_KIND_A) != 0, hb = (kind_and_flags & AMDMSM_SCAN_KIND_B) != 0;
    if (invert ? (ha || hb || (kind_and_flags & FRS_FLAG_MASK)) : (!ha && !hb)) return AMDMSM_ERR_BAD_ARG;
    if (n > FRS_MAX_N) return AMDMSM_ERR_TOO_LARGE;
    frs_layout L;
    const bool naive = frs_naive_env();
    if (!frs_make_layout(n, tile_log2, (size_t)f->words * 4, invert, naive, L)) return AMDMSM_ERR_BAD_ARG;
    out[0] = L.tile;
    out[1] = L.per_lane;
    out[2] = L.spine_step;
    out[3] = FRS_TILE_MIN;
    out[4] = FRS_TILE_MAX;
    out[5] = (size_t)L.launches;
    out[6] = L.ws_bytes;
    // reduce and apply both compose a tile's maps (a product for A, one more for B under a), apply then one per record;
    // an inversion: the tile products, the running products in a lane and two per record in the back-sweep
    const size_t fold = (ha ? 1 : 0) + (ha && hb ? 1 : 0);
    out[7] = invert ? (naive ? 3 : 4) : (naive ? (ha ? 1 : 0) : 2 * fold + (ha ? 1 : 0));
    return AMDMSM_OK;
}

int amdmsm_fr_scan_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_a, const void *a_const, const void *d_b,
                          const void *init, int flags, int tile_log2, const amdmsm_opts *opts, void *d_out, void *d_total) {
    return frs_device_entry(ctx, curve, n, d_a, a_const, d_b, init, flags, tile_log2, opts, d_out, d_total, false);
}

int amdmsm_fr_scan(amdmsm_ctx *ctx, int curve, size_t n, const void *a, const void *a_const, const void *b, const void *init,
                   int flags, int tile_log2, const amdmsm_opts *opts, void *out, void *total) {
    return frs_host_entry(ctx, curve, n, a, a_const, b, init, flags, tile_log2, opts, out, total, false);
}

int amdmsm_fr_batch_invert_device(amdmsm_ctx *ctx, int curve, size_t n, const void *d_values, int tile_log2, const amdmsm_opts *opts,
                                  void *d_out, uint64_t *d_zero_count) {
    return frs_device_entry(ctx, curve, n, d_values, nullptr, nullptr, nullptr, 0, tile_log2, opts, d_out, d_zero_count, true);
}

int amdmsm_fr_batch_invert(amdmsm_ctx *ctx, int curve, size_t n, const void *values, const amdmsm_opts *opts, void *out,
                           uint64_t *zero_count) {
    return frs_host_entry(ctx, curve, n, values, nullptr, nullptr, nullptr, 0, 0, opts, out, zero_count, true);
}

}  // extern "C"

// ---- evaluation domains over Fr: libfqfft's choice, transforms over the step radix-2 domain, division by Z --------
namespace {

// a - b mod r, both canonical
fr_rec fr_sub_host(const fr_vtable *f, const fr_rec &a, const fr_rec &b) {
    fr_rec d;
    uint64_t borrow = 0;
    for (int j = 0; j < f->words; ++j) {
        const uint64_t w = (uint64_t)a.v[j] - b.v[j] - borrow;
        d.v[j] = (uint32_t)w;
        borrow = (w >> 63) & 1u;
    }
    if (!borrow) return d;
    uint64_t carry = 0;
    for (int j = 0; j < f->words; ++j) {
        const uint64_t w = (uint64_t)d.v[j] + f->modulus[j] + carry;
        d.v[j] = (uint32_t)w;
        carry = w >> 32;
    }
    return d;
}
fr_rec fr_one(const fr_vtable *f) { return fr_from_words(f, f->one); }
fr_rec fr_neg_host(const fr_vtable *f, const fr_rec &a) { return fr_sub_host(f, fr_rec(), a); }
fr_rec fr_pow_host(const fr_vtable *f, fr_rec x, size_t e) {
    fr_rec acc = fr_one(f);
    for (; e; e >>= 1) {
        if (e & 1u) acc = fr_mul(f, acc, x);
        x = fr_mul(f, x, x);
    }
    return acc;
}
fr_rec fr_sqr_times(const fr_vtable *f, fr_rec x, int k) {
    for (int b = 0; b < k; ++b) x = fr_mul(f, x, x);
    return x;
}
// the integer k as a Montgomery residue
fr_rec fr_mont_small(const fr_vtable *f, uint32_t k) { return fr_mul(f, fr_small(k), fr_from_words(f, f->r2)); }
bool fr_is_zero(const fr_vtable *f, const fr_rec &a) { return fr_same(f, a, fr_rec()); }
// libff's get_root_of_unity(2^log2_n), Montgomery
fr_rec fr_root_host(const fr_vtable *f, int log2_n) { return fr_sqr_times(f, fr_from_words(f, f->root), f->two_adicity - log2_n); }
void fr_write(const fr_vtable *f, void *out, const fr_rec &x, bool plain) {
    const fr_rec r = plain ? fr_from_mont(f, x) : x;
    memcpy(out, r.v, (size_t)f->words * 4);
}

// A domain of m points: basic (S = 0, B = m, the points w^j, w = root(m)) or step (m = B + S: w = root(2 B), the points
// w^(2 j), j < B, then w sigma^(j - B), sigma = root(S))
struct frdom {
    bool step = false;
    size_t m = 0, B = 0, S = 0;
    int log_b = 0, log_s = 0, log_w = 0;   // log_w: log2 of the order of w
};

// libfqfft's get_evaluation_domain(min_size) as far as it ends in one of the two domains above; `why`: what went wrong
int frdom_choose(const fr_vtable *f, size_t min_size, frdom &d, std::string &why) {
    if (min_size < 2) {
        why = "min_size = " + std::to_string(min_size) + ": a domain has at least 2 points";
        return AMDMSM_ERR_BAD_ARG;
    }
    const std::string large = ": a domain of at most 2^28 points";
    if (min_size > FR_FFT_MAX_N) {
        why = "min_size = " + std::to_string(min_size) + large;
        return AMDMSM_ERR_TOO_LARGE;
    }
    const int lg = log2_exact(min_size);
    const size_t big = (size_t)1 << (lg - 1), small = min_size - big, rounded = (size_t)1 << log2_exact(small);
    d = frdom();
    if (!(min_size & (min_size - 1))) {
        d.m = min_size;
    } else if (!(small & (small - 1))) {
        d.step = true;
        d.m = min_size;
    } else if (!((big + rounded) & (big + rounded - 1))) {
        d.m = big + rounded;
    } else {
        d.step = true;
        d.m = big + rounded;
    }
    if (d.m > FR_FFT_MAX_N) {
        why = "m = " + std::to_string(d.m) + large;
        return AMDMSM_ERR_TOO_LARGE;
    }
    if (d.step) {
        d.B = big;
        d.S = d.m - big;
        d.log_b = lg - 1;
        d.log_s = log2_exact(d.S);
        d.log_w = lg;
    } else {
        d.B = d.m;
        d.log_b = d.log_w = log2_exact(d.m);
    }
    if (d.log_w > f->two_adicity) {
        // libfqfft goes on: the extended radix-2 domain serves 2^(s + 1) alone, everything else above 2^s is geometric
        const bool extended = !d.step && d.log_w == f->two_adicity + 1;
        why = "m = " + std::to_string(d.m) + ": beyond the 2-adicity " + std::to_string(f->two_adicity) + " of r - 1 libfqfft uses its " +
              (extended ? "extended radix-2" : "geometric sequence") + " domain, which is left out";
        return AMDMSM_ERR_UNSUPPORTED;
    }
    return AMDMSM_OK;
}
// the domain of exactly m points, or why there is none
int frdom_exact(const fr_vtable *f, size_t m, frdom &d, std::string &why) {
    const int rc = frdom_choose(f, m, d, why);
    if (rc || d.m == m) return rc;
    why = "m = " + std::to_string(m) + " is not a domain size: amdmsm_fr_domain chooses " + std::to_string(d.m) + " points for it";
    return AMDMSM_ERR_BAD_ARG;
}

// Workspace of a transform: the passes' own (in place, the larger of the two transforms), two vectors of partial sums
// that take turns -- at most B / 16 and B / 1024 records (frd_iters) -- the S sums of the inverse, and the two tables of
// the coset's powers.  A basic domain has the passes' alone.
struct frdom_plan {
    frdom d;
    frfft_plan pb, ps;
    size_t rec = 0, off_pa = 0, off_pb = 0, off_sums = 0, off_glo = 0, off_ghi = 0, ws_bytes = 0;
};
int frdom_make_plan(const fr_vtable *f, const frdom &d, int tile_log2, frdom_plan &p) {
    p.d = d;
    p.rec = (size_t)f->words * 4;
    if (frfft_make_plan(f, d.B, tile_log2, p.pb)) return AMDMSM_ERR_BAD_ARG;
    if (!d.step) {
        p.ws_bytes = frfft_ws_bytes(p.pb, true);
        return AMDMSM_OK;
    }
    frfft_make_plan(f, d.S, tile_log2, p.ps);
    p.off_pa = std::max(frfft_ws_bytes(p.pb, true), frfft_ws_bytes(p.ps, true));
    p.off_pb = p.off_pa + align_up(std::max<size_t>(1, d.B >> 4) * p.rec, 256);
    p.off_sums = p.off_pb + align_up(std::max<size_t>(1, d.B >> 10) * p.rec, 256);
    p.off_glo = p.off_sums + align_up(d.S * p.rec, 256);
    p.off_ghi = p.off_glo + align_up(((size_t)1 << FRD_LO_LOG2) * p.rec, 256);
    p.ws_bytes = p.off_ghi + align_up(((d.m >> FRD_LO_LOG2) + 1) * p.rec, 256);
    return AMDMSM_OK;
}

// what a transform runs with, Montgomery residues: w, the coset shift (its inverse for the inverse transform), 1 / 2, and
// the parameters of the radix-2 transforms in between
struct frdom_params {
    bool plain = false, inverse = false, has_g = false;
    fr_rec w, g, half;
    frfft_params prb, prs;
};

// The argument rules of both transform entries; nothing is launched or written and the context is not looked at before
// they hold.  device: the vectors are HBM addresses
int frdom_check(amdmsm_ctx *ctx, const fr_vtable *f, const void *values, size_t m, int flags, const void *coset, int tile_log2,
                const amdmsm_opts *opts, const void *out, bool device, frdom_plan &p, frdom_params &q, bool need_vectors = true) {
    frdom d;
    std::string why;
    int rc = frdom_exact(f, m, d, why);
    if (rc) return fail(ctx, rc, why);
    if (flags & ~AMDMSM_DOMAIN_INVERSE) return fail(ctx, AMDMSM_ERR_BAD_ARG, "flags = " + std::to_string(flags) + ": unknown bits");
    if (frdom_make_plan(f, d, tile_log2, p))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "tile_log2 = " + std::to_string(tile_log2) + ": 0 or " + std::to_string(FR_TILE_MIN) +
                                                 " .. " + std::to_string(FR_TILE_MAX));
    if (need_vectors && !values) return fail(ctx, AMDMSM_ERR_BAD_ARG, "values: null pointer");
    if (need_vectors && !out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    if (device) {
        rc = fr_check_aligned(ctx, f, "d_values / d_out", {values, out});
        if (!rc) rc = fr_check_apart(ctx, "d_values", values, m * p.rec, "d_out", out, m * p.rec);
        if (rc) return rc;
    }
    q.plain = opts && opts->scalars_plain;
    q.inverse = (flags & AMDMSM_DOMAIN_INVERSE) != 0;
    if (coset && !fr_below_modulus(f, (const uint32_t *)coset)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "coset: not below r");
    q.has_g = coset != nullptr;
    if (coset) q.g = fr_read(f, coset, q.plain);
    if (q.has_g && fr_is_zero(f, q.g)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "coset: zero");
    if (q.has_g && q.inverse) q.g = fr_inv_host(f, q.g);
    q.w = fr_root_host(f, d.log_w);
    q.half = fr_inv_host(f, fr_mont_small(f, 2));
    // the radix-2 transforms: a basic domain takes the coset as pre / post, a step domain's sweeps apply it and hold
    // Montgomery residues between themselves and the passes
    const fr_rec wi = q.inverse ? fr_inv_host(f, q.w) : q.w;
    q.prb.plain = q.prs.plain = q.plain;
    if (!d.step) {
        q.prb.omega = wi;
        q.prb.has_pre = q.has_g && !q.inverse && m > 1;
        q.prb.has_post = q.has_g && q.inverse && m > 1;
        q.prb.pre = q.prb.post = q.g;
    } else {
        q.prb.omega = fr_mul(f, wi, wi);
        q.prs.omega = fr_sqr_times(f, wi, d.log_w - d.log_s);
        q.prb.mont_in = q.prs.mont_in = !q.inverse;
        q.prb.mont_out = q.prs.mont_out = q.inverse;
    }
    q.prb.scale = q.prs.scale = fr_one(f);
    if (q.inverse) {
        q.prb.has_scale = true;
        q.prb.scale = fr_inv_host(f, fr_mont_small(f, (uint32_t)d.B));
        q.prs.has_scale = d.step;
        if (d.step) q.prs.scale = fr_inv_host(f, fr_mont_small(f, (uint32_t)d.S));
    }
    return AMDMSM_OK;
}

// the sweep over the K x S matrix and, launch after launch, over the rows of partial sums it leaves; the last launch
// writes the S sums to `final`
void frdom_sweeps(const fr_vtable *f, hipStream_t st, const frdom_plan &p, frd_sweep a, uint32_t *final, char *ws) {
    uint32_t *turn[2] = {(uint32_t *)(ws + p.off_pa), (uint32_t *)(ws + p.off_pb)};
    a.log_b = p.d.log_b;
    a.log_s = p.d.log_s;
    a.log_w = std::min(p.d.log_s, FRD_TILE_LOG2);
    a.rows = (uint32_t)(p.d.B >> p.d.log_s);
    a.iters = frd_iters(a.log_w);
    for (int k = 0;; k ^= 1) {
        const uint32_t per = (256u >> a.log_w) * a.iters, left = (a.rows + per - 1) / per;
        a.sums = left == 1 ? final : turn[k];
        f->domain_sweep(st, a);
        if (left == 1) return;
        a.in = a.sums;
        a.mode = FRD_REDUCE;
        a.rows = left;
        a.iters = FRD_ITERS_REDUCE;
    }
}

// The transform on device-resident vectors, d_out == d_in or apart; ws: frdom_plan's workspace.  Phase 0 builds every
// table of powers the call reads, phase 1 is the sweeps and the passes.
int frdom_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frdom_plan &p, const frdom_params &q, const uint32_t *d_in,
              uint32_t *d_out, char *ws) {
    const frdom &d = p.d;
    if (!d.step) return frfft_run(ctx, f, st, p.pb, q.prb, d_in, d_out, d.m, ws);
    const size_t nw = (size_t)f->words;
    fr_tw_entry *tw = nullptr, *pre = nullptr;
    frfft_params pw;
    pw.omega = q.w;
    int rc = frfft_twiddles(ctx, f, st, 2 * d.B, pw, tw);   // the B powers of w: the fold's and the merge's factors
    // the passes' own powers now, so that they fall into phase 0; frfft_run finds them again
    if (!rc && d.B > 1) rc = frfft_twiddles(ctx, f, st, d.B, q.prb, pre);
    if (!rc && d.S > 1) rc = frfft_twiddles(ctx, f, st, d.S, q.prs, pre);
    if (rc) return rc;
    uint32_t *g_lo = nullptr, *g_hi = nullptr;
    if (q.has_g) {
        g_lo = (uint32_t *)(ws + p.off_glo);
        g_hi = (uint32_t *)(ws + p.off_ghi);
        f->powers(st, fr_pow_table(f, q.g, 0).data(), nullptr, 0, (size_t)1 << FRD_LO_LOG2, g_lo);
        f->powers(st, fr_pow_table(f, q.g, FRD_LO_LOG2).data(), nullptr, 0, (d.m >> FRD_LO_LOG2) + 1, g_hi);
    }
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 1);
    frd_sweep a = {};
    a.tw = (const uint32_t *)tw->buf.p;
    a.g_lo = g_lo;
    a.g_hi = g_hi;
    a.plain = q.plain ? 1 : 0;
    uint32_t *hi = d_out + d.B * nw;
    if (!q.inverse) {
        // c to d_out[0 .. B) -- a lane reads the records i and B + i before it writes record i, and no other lane reads
        // them, so d_out may be d_in -- the sums e to d_out[B .. m), then both transforms in place
        a.mode = FRD_FOLD;
        a.in = d_in;
        a.out = d_out;
        a.store = (d_in != d_out || q.plain || q.has_g) ? 1 : 0;
        frdom_sweeps(f, st, p, a, hi, ws);
        HIP_TRY(ctx, hipGetLastError());
        rc = frfft_run(ctx, f, st, p.pb, q.prb, d_out, d_out, d.B, ws);
        if (!rc) rc = frfft_run(ctx, f, st, p.ps, q.prs, hi, hi, d.S, ws);
        if (rc) return rc;
    } else {
        rc = frfft_run(ctx, f, st, p.pb, q.prb, d_in, d_out, d.B, ws);
        if (!rc) rc = frfft_run(ctx, f, st, p.ps, q.prs, d_in + d.B * nw, hi, d.S, ws);
        if (rc) return rc;
        uint32_t *sums = (uint32_t *)(ws + p.off_sums);
        a.mode = FRD_MERGE;
        a.in = d_out;
        a.out = d_out;
        a.store = (q.plain || q.has_g) ? 1 : 0;
        frdom_sweeps(f, st, p, a, sums, ws);
        frd_combine c = {};
        c.out = d_out;
        c.sums = sums;
        c.tw = a.tw;
        c.g_lo = g_lo;
        c.g_hi = g_hi;
        c.log_b = d.log_b;
        c.log_s = d.log_s;
        c.plain = a.plain;
        memcpy(c.half, q.half.v, sizeof(c.half));
        f->domain_combine(st, c);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(tw->ev, st));
    return AMDMSM_OK;
}

// ---- division by Z on the coset g D: out[j] = values[j] / Z(g x_j) --------------------------------------------------------
// Step domain: below B the denominator (g^B - 1) (g^S rho^j - w^S), rho = w^(2 S) of order K, takes K values -- built as
// powers of rho, inverted by the batch inversion of section 20 and indexed by j mod K; from B on it is the one value
// -(g^B + 1) w^S (g^S - 1), inverted here.  Basic domain: g^m - 1 throughout.
struct frdiv_call {
    frdom d;
    size_t rec = 0, K = 0, off_scan = 0, ws_bytes = 0;
    bool plain = false;
    fr_rec rho, first, sub, tail;   // den[k] = first rho^k - sub
    frs_call inv;
};
int frdiv_check(amdmsm_ctx *ctx, const fr_vtable *f, size_t m, const void *values, const void *coset, const amdmsm_opts *opts,
                const void *out, bool device, frdiv_call &c) {
    std::string why;
    int rc = frdom_exact(f, m, c.d, why);
    if (rc) return fail(ctx, rc, why);
    c.rec = (size_t)f->words * 4;
    if (!values) return fail(ctx, AMDMSM_ERR_BAD_ARG, "values: null pointer");
    if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    if (!coset) return fail(ctx, AMDMSM_ERR_BAD_ARG, "coset: null pointer (Z is zero on the domain itself)");
    if (device) {
        rc = fr_check_aligned(ctx, f, "d_values / d_out", {values, out});
        if (!rc) rc = fr_check_apart(ctx, "d_values", values, m * c.rec, "d_out", out, m * c.rec);
        if (rc) return rc;
    }
    c.plain = opts && opts->scalars_plain;
    if (!fr_below_modulus(f, (const uint32_t *)coset)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "coset: not below r");
    const frdom &d = c.d;
    const fr_rec g = fr_read(f, coset, c.plain), one = fr_one(f);
    const fr_rec gb = fr_pow_host(f, g, d.B);
    const size_t order = d.step ? 2 * d.B : d.m;
    if (fr_same(f, fr_pow_host(f, g, order), one))
        return fail(ctx, AMDMSM_ERR_BAD_ARG, "coset: g^" + std::to_string(order) + " = 1, Z has a zero on the coset");
    if (!d.step) {
        c.tail = fr_inv_host(f, fr_sub_host(f, gb, one));
        return AMDMSM_OK;
    }
    c.K = d.B >> d.log_s;
    const fr_rec w = fr_root_host(f, d.log_w), ws = fr_pow_host(f, w, d.S), gs = fr_pow_host(f, g, d.S);
    const fr_rec lead = fr_sub_host(f, gb, one);
    c.rho = fr_mul(f, ws, ws);
    c.first = fr_mul(f, lead, gs);
    c.sub = fr_mul(f, lead, ws);
    // (g w sigma^t)^B - 1 = -g^B - 1 and (g w sigma^t)^S - w^S = w^S (g^S - 1)
    const fr_rec tail = fr_mul(f, fr_neg_host(f, fr_sub_host(f, gb, fr_neg_host(f, one))), fr_mul(f, ws, fr_sub_host(f, gs, one)));
    c.tail = fr_inv_host(f, tail);
    // the K denominators and their inversion in place, Montgomery residues whatever the caller's records are
    c.inv.rec = c.rec;
    c.inv.invert = true;
    c.inv.naive = frs_naive_env();
    c.inv.has_a = 1;
    frs_make_layout(c.K, 0, c.rec, true, c.inv.naive, c.inv.L);
    c.off_scan = align_up(c.K * c.rec, 256);
    c.ws_bytes = c.off_scan + c.inv.L.ws_bytes;
    return AMDMSM_OK;
}
int frdiv_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frdiv_call &c, const uint32_t *d_in, uint32_t *d_out, char *ws) {
    const frdom &d = c.d;
    uint32_t *den = (uint32_t *)ws;
    if (d.step) {
        f->powers(st, fr_pow_table(f, c.rho, 0).data(), c.first.v, 0, c.K, den);
        f->domain_den(st, c.K, den, c.sub.v);
        HIP_TRY(ctx, hipGetLastError());
        const int rc = frs_run(ctx, f, st, c.inv, c.K, den, nullptr, den, nullptr, ws + c.off_scan);   // marks phase 1
        if (rc) return rc;
    } else {
        call_mark(ctx, st, 1);
    }
    f->domain_divide(st, d.m, d.step ? d.B : 0, c.K, d_in, den, c.tail.v, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

// ---- the Lagrange vector of a domain at a point: out[j] = L_j(t) ---------------------------------------------
// With Z = Z(t) != 0 the denominators are
//     basic:           1 / L_j = (t / x_j - 1) m / Z
//     step, j < B:     1 / L_j = (t / x_j - 1) B (rho^(j mod K) - w^S) / Z,   rho = w^(2 S) of order K
//     step, j >= B:    1 / L_j = (t / x_j - 1) (-2 S w^S) / Z
// one sweep writes them and the batch inversion of section 20 inverts them in place.  The K factors below B are built as
// frdiv_run builds its own: powers of rho, then a subtraction.  The inversion takes and leaves Montgomery residues; for
// plain results the factors carry one more R, so that what it leaves is the plain integer.  Z = 0: t is a point of the
// domain and the sweep writes the unit vector.
struct frlag_call {
    frdom d;
    size_t rec = 0, K = 0, off_scan = 0, ws_bytes = 0;
    bool plain = false, unit = false;
    fr_rec w, t, rho, first, sub, tail;   // kden[k] = first rho^k - sub
    frs_call inv;
};
int frlag_check(amdmsm_ctx *ctx, const fr_vtable *f, size_t m, const void *t, const amdmsm_opts *opts, const void *out, bool device,
                frlag_call &c) {
    std::string why;
    int rc = frdom_exact(f, m, c.d, why);
    if (rc) return fail(ctx, rc, why);
    c.rec = (size_t)f->words * 4;
    if (!t) return fail(ctx, AMDMSM_ERR_BAD_ARG, "t: null pointer");
    if (!out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "output: null pointer");
    if (device) {
        rc = fr_check_aligned(ctx, f, "d_out", {out});
        if (rc) return rc;
    }
    if (!fr_below_modulus(f, (const uint32_t *)t)) return fail(ctx, AMDMSM_ERR_BAD_ARG, "t: not below r");
    c.plain = opts && opts->scalars_plain;
    const frdom &d = c.d;
    const fr_rec one = fr_one(f), r2 = fr_from_words(f, f->r2);
    c.t = fr_read(f, t, c.plain);
    c.w = fr_root_host(f, d.log_w);
    const fr_rec ws = fr_pow_host(f, c.w, d.S);
    fr_rec z = fr_sub_host(f, fr_pow_host(f, c.t, d.B), one);
    if (d.step) z = fr_mul(f, z, fr_sub_host(f, fr_pow_host(f, c.t, d.S), ws));
    c.unit = fr_is_zero(f, z);
    if (c.unit) {
        c.tail = c.plain ? fr_small(1) : one;
        return AMDMSM_OK;
    }
    const fr_rec zi = fr_inv_host(f, z);
    if (!d.step) {
        c.tail = fr_mul(f, fr_mont_small(f, (uint32_t)d.m), zi);
    } else {
        c.K = d.B >> d.log_s;
        c.rho = fr_mul(f, ws, ws);
        c.first = fr_mul(f, fr_mont_small(f, (uint32_t)d.B), zi);
        c.sub = fr_mul(f, c.first, ws);
        c.tail = fr_neg_host(f, fr_mul(f, fr_mul(f, fr_mont_small(f, (uint32_t)(2 * d.S)), ws), zi));
    }
    if (c.plain) {
        c.first = fr_mul(f, c.first, r2);
        c.sub = fr_mul(f, c.sub, r2);
        c.tail = fr_mul(f, c.tail, r2);
    }
    c.inv.rec = c.rec;
    c.inv.invert = true;
    c.inv.naive = frs_naive_env();
    c.inv.has_a = 1;
    frs_make_layout(m, 0, c.rec, true, c.inv.naive, c.inv.L);
    c.off_scan = align_up(c.K * c.rec, 256);
    c.ws_bytes = c.off_scan + c.inv.L.ws_bytes;
    return AMDMSM_OK;
}
// phase 0: the powers of w, from the context's cache or built now, and the K factors; phase 1: the sweep and the inversion
int frlag_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frlag_call &c, uint32_t *d_out, char *ws) {
    const frdom &d = c.d;
    fr_tw_entry *tw = nullptr;
    frfft_params pw;
    pw.omega = c.w;
    const int rc = frfft_twiddles(ctx, f, st, (size_t)1 << d.log_w, pw, tw);
    if (rc) return rc;
    uint32_t *kden = (uint32_t *)ws;
    if (d.step && !c.unit) {
        f->powers(st, fr_pow_table(f, c.rho, 0).data(), c.first.v, 0, c.K, kden);
        f->domain_den(st, c.K, kden, c.sub.v);
    }
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 1);
    frd_lagrange a = {};
    a.tw = (const uint32_t *)tw->buf.p;
    a.kden = kden;
    a.out = d_out;
    a.m = d.m;
    a.log_b = d.log_b;
    a.log_s = d.log_s;
    a.log_o = d.log_w;
    a.step = d.step ? 1 : 0;
    a.unit = c.unit ? 1 : 0;
    memcpy(a.t, c.t.v, sizeof(a.t));
    memcpy(a.tail, c.tail.v, sizeof(a.tail));
    f->domain_lagrange(st, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(tw->ev, st));
    if (c.unit) return AMDMSM_OK;
    return frs_run(ctx, f, st, c.inv, d.m, d_out, nullptr, d_out, nullptr, ws + c.off_scan);
}

}   // namespace

extern "C" {

int amdmsm_fr_domain(int curve, size_t min_size, size_t out[6]) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out) return AMDMSM_ERR_BAD_ARG;
    frdom d;
    std::string why;
    const int rc = frdom_choose(f, min_size, d, why);
    if (rc) return rc;
    frdom_plan p;
    frdom_make_plan(f, d, 0, p);
    out[0] = d.step ? AMDMSM_DOMAIN_STEP_RADIX2 : AMDMSM_DOMAIN_BASIC_RADIX2;
    out[1] = d.m;
    out[2] = d.B;
    out[3] = d.S;
    out[4] = (size_t)d.log_w;
    out[5] = p.ws_bytes;
    return AMDMSM_OK;
}

int amdmsm_fr_domain_element(int curve, size_t m, size_t idx, int plain, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    frdom d;
    std::string why;
    const int rc = frdom_exact(f, m, d, why);
    if (rc) return rc;
    if (!out || idx >= m) return AMDMSM_ERR_BAD_ARG;
    const fr_rec w = fr_root_host(f, d.log_w);
    fr_rec x;
    if (!d.step) x = fr_pow_host(f, w, idx);
    else if (idx < d.B) x = fr_pow_host(f, w, 2 * idx);
    else x = fr_mul(f, w, fr_pow_host(f, fr_root_host(f, d.log_s), idx - d.B));
    fr_write(f, out, x, plain != 0);
    return AMDMSM_OK;
}

int amdmsm_fr_domain_vanishing(int curve, size_t m, const void *t, int plain, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    frdom d;
    std::string why;
    const int rc = frdom_exact(f, m, d, why);
    if (rc) return rc;
    if (!t || !out || !fr_below_modulus(f, (const uint32_t *)t)) return AMDMSM_ERR_BAD_ARG;
    const fr_rec x = fr_read(f, t, plain != 0), one = fr_one(f);
    fr_rec z = fr_sub_host(f, fr_pow_host(f, x, d.B), one);
    if (d.step) z = fr_mul(f, z, fr_sub_host(f, fr_pow_host(f, x, d.S), fr_pow_host(f, fr_root_host(f, d.log_w), d.S)));
    fr_write(f, out, z, plain != 0);
    return AMDMSM_OK;
}

int amdmsm_fr_domain_z_terms(int curve, size_t m, int plain, size_t idx[4], void *coeffs, int *count) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    frdom d;
    std::string why;
    const int rc = frdom_exact(f, m, d, why);
    if (rc) return rc;
    if (!idx || !coeffs || !count) return AMDMSM_ERR_BAD_ARG;
    const fr_rec one = fr_one(f), minus_one = fr_neg_host(f, one);
    const size_t rec = (size_t)f->words * 4;
    char *c = (char *)coeffs;
    if (!d.step) {   // X^m - 1
        idx[0] = m;
        idx[1] = 0;
        fr_write(f, c, one, plain != 0);
        fr_write(f, c + rec, minus_one, plain != 0);
        *count = 2;
        return AMDMSM_OK;
    }
    // (X^B - 1) (X^S - w^S) = X^(B+S) - w^S X^B - X^S + w^S
    const fr_rec ws = fr_pow_host(f, fr_root_host(f, d.log_w), d.S);
    idx[0] = d.B + d.S;
    idx[1] = d.B;
    idx[2] = d.S;
    idx[3] = 0;
    fr_write(f, c, one, plain != 0);
    fr_write(f, c + rec, fr_neg_host(f, ws), plain != 0);
    fr_write(f, c + 2 * rec, minus_one, plain != 0);
    fr_write(f, c + 3 * rec, ws, plain != 0);
    *count = 4;
    return AMDMSM_OK;
}

int amdmsm_fr_multiplicative_generator(int curve, int plain, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out) return AMDMSM_ERR_BAD_ARG;
    fr_write(f, out, fr_from_words(f, f->generator), plain != 0);
    return AMDMSM_OK;
}

int amdmsm_fr_domain_fft_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t m, int flags, const void *coset,
                                int tile_log2, const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frdom_plan p;
    frdom_params q;
    const int rc = frdom_check(ctx, f, d_values, m, flags, coset, tile_log2, opts, d_out, true, p, q);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, p.ws_bytes, {}, {}, [&](char *, char *ws) {
        return frdom_run(ctx, f, st, p, q, (const uint32_t *)d_values, (uint32_t *)d_out, ws);
    });
}

int amdmsm_fr_domain_fft(amdmsm_ctx *ctx, int curve, const void *values, size_t m, int flags, const void *coset, int tile_log2,
                         const amdmsm_opts *opts, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frdom_plan p;
    frdom_params q;
    const int rc = frdom_check(ctx, f, values, m, flags, coset, tile_log2, opts, out, false, p, q);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = ctx->stream;
    // one staged vector; the transform runs in place on it
    const size_t vec = align_up(m * p.rec, 256);
    return fr_call(ctx, st, vec, p.ws_bytes, {{values, 0, m * p.rec}}, {{out, 0, m * p.rec}}, [&](char *v, char *ws) {
        return frdom_run(ctx, f, st, p, q, (const uint32_t *)v, (uint32_t *)v, ws);
    });
}

int amdmsm_fr_domain_divide_by_z_device(amdmsm_ctx *ctx, int curve, size_t m, const void *d_values, const void *coset,
                                        const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frdiv_call c;
    const int rc = frdiv_check(ctx, f, m, d_values, coset, opts, d_out, true, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, std::max<size_t>(c.ws_bytes, 256), {}, {}, [&](char *, char *ws) {
        return frdiv_run(ctx, f, st, c, (const uint32_t *)d_values, (uint32_t *)d_out, ws);
    });
}

int amdmsm_fr_domain_divide_by_z(amdmsm_ctx *ctx, int curve, size_t m, const void *values, const void *coset,
                                 const amdmsm_opts *opts, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frdiv_call c;
    const int rc = frdiv_check(ctx, f, m, values, coset, opts, out, false, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const size_t vec = align_up(m * c.rec, 256);
    return fr_call(ctx, st, vec, std::max<size_t>(c.ws_bytes, 256), {{values, 0, m * c.rec}}, {{out, 0, m * c.rec}},
                   [&](char *v, char *ws) { return frdiv_run(ctx, f, st, c, (const uint32_t *)v, (uint32_t *)v, ws); });
}

int amdmsm_fr_domain_lagrange_device(amdmsm_ctx *ctx, int curve, size_t m, const void *t, const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frlag_call c;
    const int rc = frlag_check(ctx, f, m, t, opts, d_out, true, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, std::max<size_t>(c.ws_bytes, 256), {}, {},
                   [&](char *, char *ws) { return frlag_run(ctx, f, st, c, (uint32_t *)d_out, ws); });
}

int amdmsm_fr_domain_lagrange(amdmsm_ctx *ctx, int curve, size_t m, const void *t, const amdmsm_opts *opts, void *out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frlag_call c;
    const int rc = frlag_check(ctx, f, m, t, opts, out, false, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    hipStream_t st = ctx->stream;
    // one staged vector, written by the sweep and inverted in place; nothing goes up
    const size_t vec = align_up(m * c.rec, 256);
    return fr_call(ctx, st, vec, std::max<size_t>(c.ws_bytes, 256), {}, {{out, 0, m * c.rec}},
                   [&](char *v, char *ws) { return frlag_run(ctx, f, st, c, (uint32_t *)v, ws); });
}

int amdmsm_fr_lincomb_device(amdmsm_ctx *ctx, int curve, size_t n, int k, const void *const *d_v, const void *scalars,
                             const amdmsm_opts *opts, void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    if (k < 1 || k > FR_LINCOMB_MAX) return fail(ctx, AMDMSM_ERR_BAD_ARG, "k = " + std::to_string(k) + ": 1 .. " + std::to_string(FR_LINCOMB_MAX));
    if (n > FRS_MAX_N) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n = " + std::to_string(n) + ": at most 2^28 records");
    if (!d_v) return fail(ctx, AMDMSM_ERR_BAD_ARG, "d_v: null pointer");
    if (!scalars) return fail(ctx, AMDMSM_ERR_BAD_ARG, "scalars: null pointer");
    const size_t rec = (size_t)f->words * 4, bytes = n * rec;
    if (n && !d_out) return fail(ctx, AMDMSM_ERR_BAD_ARG, "d_out: null pointer");
    for (int j = 0; j < k; ++j) {
        const std::string name = "d_v[" + std::to_string(j) + "]";
        if (n && !d_v[j]) return fail(ctx, AMDMSM_ERR_BAD_ARG, name + ": null pointer");
        int rc = n ? fr_check_aligned(ctx, f, "d_v / d_out", {d_v[j], d_out}) : AMDMSM_OK;
        if (!rc) rc = fr_check_apart(ctx, name.c_str(), d_v[j], bytes, "d_out", d_out, bytes);
        if (rc) return rc;
        if (!fr_below_modulus(f, (const uint32_t *)((const char *)scalars + j * rec)))
            return fail(ctx, AMDMSM_ERR_BAD_ARG, "scalars[" + std::to_string(j) + "]: not below r");
    }
    FR_ENTER(ctx);
    if (!n) return AMDMSM_OK;
    const bool plain = opts && opts->scalars_plain;
    uint32_t s[FR_LINCOMB_MAX * FR_MAX_WORDS] = {};
    for (int j = 0; j < k; ++j) memcpy(s + (size_t)j * f->words, fr_read(f, (const char *)scalars + j * rec, plain).v, rec);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, 256, {}, {}, [&](char *, char *) -> int {
        call_mark(ctx, st, 1);
        f->lincomb(st, n, k, (const uint32_t *const *)d_v, s, (uint32_t *)d_out);
        HIP_TRY(ctx, hipGetLastError());
        return AMDMSM_OK;
    });
}

}  // extern "C"

// ---- batched transforms over a domain, and the R1CS-to-QAP witness map as one call -----------------------------
namespace {

// A batch over one domain.  Basic: the batched passes.  Step: the radix-2 transforms of B and of S records go through the
// batched passes -- vector v's B records at v stride, its S records B records further on -- and the fold, merge and
// combine sweeps run vector by vector with the kernels of one vector, in stream order on one set of partial sums.
// Workspace: the passes' (in place, the larger of the two batches), then the sweeps' regions of frdom_plan, `shift`
// bytes further on than one vector has them.
struct frdom_batch_plan {
    frdom_plan p;
    frfft_batch_plan bb, bs;
    size_t batch = 0, shift = 0, ws_bytes = 0;
};
void frdom_make_batch_plan(const frdom_plan &p, size_t batch, frdom_batch_plan &b) {
    b.p = p;
    b.batch = batch;
    frfft_make_batch_plan(p.pb, p.d.B, batch, b.bb);
    if (!p.d.step) {
        b.ws_bytes = frfft_batch_ws_bytes(b.bb, true);
        return;
    }
    frfft_make_batch_plan(p.ps, p.d.S, batch, b.bs);
    b.shift = std::max(frfft_batch_ws_bytes(b.bb, true), frfft_batch_ws_bytes(b.bs, true)) - p.off_pa;
    b.ws_bytes = p.ws_bytes + b.shift;
}

// frdom_run over a batch, batch >= 1: vector v at d_in + v in_stride records and d_out + v out_stride records
int frdom_run_batch(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frdom_batch_plan &b, const frdom_params &q,
                    const uint32_t *d_in, size_t in_stride, uint32_t *d_out, size_t out_stride, char *ws) {
    const frdom_plan &p = b.p;
    const frdom &d = p.d;
    if (!d.step) return frfft_run_batch(ctx, f, st, b.bb, q.prb, d_in, in_stride, d_out, out_stride, d.m, ws);
    const size_t nw = (size_t)f->words;
    fr_tw_entry *tw = nullptr, *pre = nullptr;
    frfft_params pw;
    pw.omega = q.w;
    int rc = frfft_twiddles(ctx, f, st, 2 * d.B, pw, tw);
    if (!rc && d.B > 1) rc = frfft_twiddles(ctx, f, st, d.B, q.prb, pre);
    if (!rc && d.S > 1) rc = frfft_twiddles(ctx, f, st, d.S, q.prs, pre);
    if (rc) return rc;
    char *sweeps = ws + b.shift;   // where the sweeps find frdom_plan's regions
    uint32_t *g_lo = nullptr, *g_hi = nullptr;
    if (q.has_g) {
        g_lo = (uint32_t *)(sweeps + p.off_glo);
        g_hi = (uint32_t *)(sweeps + p.off_ghi);
        f->powers(st, fr_pow_table(f, q.g, 0).data(), nullptr, 0, (size_t)1 << FRD_LO_LOG2, g_lo);
        f->powers(st, fr_pow_table(f, q.g, FRD_LO_LOG2).data(), nullptr, 0, (d.m >> FRD_LO_LOG2) + 1, g_hi);
    }
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 1);
    frd_sweep a = {};
    a.tw = (const uint32_t *)tw->buf.p;
    a.g_lo = g_lo;
    a.g_hi = g_hi;
    a.plain = q.plain ? 1 : 0;
    uint32_t *hi = d_out + d.B * nw;
    if (!q.inverse) {
        a.mode = FRD_FOLD;
        a.store = (d_in != d_out || q.plain || q.has_g) ? 1 : 0;
        for (size_t v = 0; v < b.batch; ++v) {
            a.in = d_in + v * in_stride * nw;
            a.out = d_out + v * out_stride * nw;
            frdom_sweeps(f, st, p, a, hi + v * out_stride * nw, sweeps);
        }
        HIP_TRY(ctx, hipGetLastError());
        rc = frfft_run_batch(ctx, f, st, b.bb, q.prb, d_out, out_stride, d_out, out_stride, d.B, ws);
        if (!rc) rc = frfft_run_batch(ctx, f, st, b.bs, q.prs, hi, out_stride, hi, out_stride, d.S, ws);
        if (rc) return rc;
    } else {
        rc = frfft_run_batch(ctx, f, st, b.bb, q.prb, d_in, in_stride, d_out, out_stride, d.B, ws);
        if (!rc) rc = frfft_run_batch(ctx, f, st, b.bs, q.prs, d_in + d.B * nw, in_stride, hi, out_stride, d.S, ws);
        if (rc) return rc;
        uint32_t *sums = (uint32_t *)(sweeps + p.off_sums);
        a.mode = FRD_MERGE;
        a.store = (q.plain || q.has_g) ? 1 : 0;
        frd_combine c = {};
        c.sums = sums;
        c.tw = a.tw;
        c.g_lo = g_lo;
        c.g_hi = g_hi;
        c.log_b = d.log_b;
        c.log_s = d.log_s;
        c.plain = a.plain;
        memcpy(c.half, q.half.v, sizeof(c.half));
        for (size_t v = 0; v < b.batch; ++v) {
            a.in = a.out = c.out = d_out + v * out_stride * nw;
            frdom_sweeps(f, st, p, a, sums, sweeps);
            f->domain_combine(st, c);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(tw->ev, st));
    return AMDMSM_OK;
}

// What a witness map runs with.  The workspace: the three vectors aA, aB, aC of m records, packed; the partial sums of an
// apply; the batch transform's workspace, which serves the single inverse coset transform too; the division's.
struct frqap_call {
    frdom_plan dp;
    frdom_batch_plan bp;
    frdom_params inv, cos, icos;   // the inverse transform, the coset transform, the inverse coset transform
    frdiv_call div;
    fr_matrix *mat[3] = {};
    bool plain = false, blind = false;
    fr_rec d1, d2;                 // Montgomery
    fr_terms terms = {};           // h[m], and with blinding d1 d2 Z - d3
    size_t rec = 0, off_part = 0, off_tr = 0, off_div = 0, ws_bytes = 0;
};

// The rules that need no context: the domain, the vectors, the blinding.  z and h are HBM addresses with `device`.
int frqap_check(amdmsm_ctx *ctx, const fr_vtable *f, const void *z, size_t n_z, size_t m, const void *blind, const amdmsm_opts *opts,
                const void *h, bool device, frqap_call &c) {
    c.rec = (size_t)f->words * 4;
    c.plain = opts && opts->scalars_plain;
    c.blind = blind != nullptr;
    // the coset of the quotient in the caller's form; the three transforms' own rules give the domain's refusals
    uint32_t g[FR_MAX_WORDS] = {};
    fr_write(f, g, fr_from_words(f, f->generator), c.plain);
    int rc = frdom_check(ctx, f, nullptr, m, AMDMSM_DOMAIN_INVERSE, nullptr, 0, opts, nullptr, false, c.dp, c.inv, false);
    if (rc) return rc;
    if (n_z > FRM_MAX_DIM) return fail(ctx, AMDMSM_ERR_TOO_LARGE, "n_z = " + std::to_string(n_z) + ": at most 2^28 records");
    if (n_z && !z) return fail(ctx, AMDMSM_ERR_BAD_ARG, device ? "d_z: null pointer" : "z: null pointer");
    if (!h) return fail(ctx, AMDMSM_ERR_BAD_ARG, device ? "d_h: null pointer" : "h: null pointer");
    if (device) {
        rc = fr_check_aligned(ctx, f, "d_z / d_h", {z, h});
        if (!rc) rc = fr_check_apart(ctx, "d_z", z, n_z * c.rec, "d_h", h, (m + 1) * c.rec, false);
        if (rc) return rc;
    }
    fr_rec d3;
    if (c.blind) {
        for (int k = 0; k < 3; ++k)
            if (!fr_below_modulus(f, (const uint32_t *)((const char *)blind + k * c.rec)))
                return fail(ctx, AMDMSM_ERR_BAD_ARG, "blind[" + std::to_string(k) + "]: not below r");
        c.d1 = fr_read(f, blind, c.plain);
        c.d2 = fr_read(f, (const char *)blind + c.rec, c.plain);
        d3 = fr_read(f, (const char *)blind + 2 * c.rec, c.plain);
    }
    rc = frdom_check(ctx, f, nullptr, m, 0, g, 0, opts, nullptr, false, c.dp, c.cos, false);
    if (!rc) rc = frdom_check(ctx, f, nullptr, m, AMDMSM_DOMAIN_INVERSE, g, 0, opts, nullptr, false, c.dp, c.icos, false);
    if (!rc) rc = frdiv_check(ctx, f, m, g, g, opts, g, false, c.div);   // no vectors yet: any non-null address
    if (rc) return rc;
    frdom_make_batch_plan(c.dp, 3, c.bp);
    // h[m] = d1 d2 (0 without blinding), stored; with blinding the other terms of d1 d2 Z, and -d3 with the constant one
    c.terms.idx[0] = m;
    c.terms.count = 1;
    c.terms.set = 1;
    if (c.blind) {
        uint32_t coef[FR_TERMS_MAX][FR_MAX_WORDS] = {};
        std::vector<uint32_t> packed((size_t)FR_TERMS_MAX * f->words);
        if (amdmsm_fr_domain_z_terms(f->curve, m, 0, c.terms.idx, packed.data(), &c.terms.count)) return AMDMSM_ERR_BAD_ARG;
        const fr_rec dd = fr_mul(f, c.d1, c.d2);
        for (int k = 0; k < c.terms.count; ++k) {
            fr_rec t = fr_mul(f, dd, fr_from_words(f, &packed[(size_t)k * f->words]));
            if (c.terms.idx[k] == 0) t = fr_sub_host(f, t, d3);
            fr_write(f, coef[k], t, c.plain);
        }
        memcpy(c.terms.c, coef, sizeof(coef));
    }
    return AMDMSM_OK;
}

// The rules of the three handles, with the context held, and the workspace
int frqap_handles(amdmsm_ctx *ctx, const fr_vtable *f, const uint64_t mats[3], size_t n_z, size_t m, frqap_call &c) {
    const char *names[3] = {"mat_a", "mat_b", "mat_c"};
    size_t part = 256;
    for (int j = 0; j < 3; ++j) {
        fr_matrix *mt = frm_find(ctx, mats[j]);
        if (!mt)
            return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(names[j]) + ": matrix handle " + std::to_string(mats[j]) + ": not a live handle of this context");
        if (mt->curve != f->curve) return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(names[j]) + ": a matrix of another curve");
        if (mt->n_rows > m)
            return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(names[j]) + ": n_rows = " + std::to_string(mt->n_rows) + " > m = " + std::to_string(m));
        if (n_z < mt->n_cols)
            return fail(ctx, AMDMSM_ERR_BAD_ARG, std::string(names[j]) + ": n_z = " + std::to_string(n_z) + " < n_cols = " + std::to_string(mt->n_cols));
        c.mat[j] = mt;
        part = std::max(part, frm_ws_bytes(f, mt));
    }
    c.off_part = align_up(3 * m * c.rec, 256);
    c.off_tr = c.off_part + part;
    c.off_div = c.off_tr + c.bp.ws_bytes;
    c.ws_bytes = c.off_div + std::max<size_t>(c.div.ws_bytes, 256);
    return AMDMSM_OK;
}

// every kernel of the map, in stream order; ws: frqap_call's workspace
int frqap_run(amdmsm_ctx *ctx, const fr_vtable *f, hipStream_t st, const frqap_call &c, const uint32_t *d_z, uint32_t *d_h, char *ws) {
    const size_t m = c.dp.d.m, nw = (size_t)f->words;
    uint32_t *v[3] = {(uint32_t *)ws, (uint32_t *)ws + m * nw, (uint32_t *)ws + 2 * m * nw};
    char *tr = ws + c.off_tr;
    int rc = AMDMSM_OK;
    for (int j = 0; j < 3 && !rc; ++j) rc = frm_run(ctx, f, st, c.mat[j], d_z, v[j], m, (uint32_t *)(ws + c.off_part));
    if (rc) return rc;
    call_mark(ctx, st, 0);   // the tables of a transform belong to phase 0, here and below
    rc = frdom_run_batch(ctx, f, st, c.bp, c.inv, v[0], m, v[0], m, tr);
    if (rc) return rc;
    const fr_rec one = fr_one(f);
    uint32_t s[2 * FR_MAX_WORDS] = {};
    if (c.blind) {   // d2 A + d1 B, while A and B are coefficients
        memcpy(s, c.d2.v, nw * 4);
        memcpy(s + nw, c.d1.v, nw * 4);
        const uint32_t *ab[2] = {v[0], v[1]};
        f->lincomb(st, m, 2, ab, s, d_h);
    }
    call_mark(ctx, st, 0);
    rc = frdom_run_batch(ctx, f, st, c.bp, c.cos, v[0], m, v[0], m, tr);
    if (rc) return rc;
    f->muladd(st, m, v[0], v[1], v[2], nullptr, c.plain ? 1 : 0, v[0]);
    HIP_TRY(ctx, hipGetLastError());
    call_mark(ctx, st, 0);
    rc = frdiv_run(ctx, f, st, c.div, v[0], v[0], ws + c.off_div);
    if (rc) return rc;
    call_mark(ctx, st, 0);
    rc = frdom_run(ctx, f, st, c.dp, c.icos, v[0], c.blind ? v[0] : d_h, tr);
    if (rc) return rc;
    if (c.blind) {
        memcpy(s, one.v, nw * 4);
        memcpy(s + nw, one.v, nw * 4);
        const uint32_t *qh[2] = {v[0], d_h};
        f->lincomb(st, m, 2, qh, s, d_h);
    }
    f->add_terms(st, c.terms, d_h);
    HIP_TRY(ctx, hipGetLastError());
    return AMDMSM_OK;
}

}   // namespace

extern "C" {

int amdmsm_fr_domain_fft_batch_device(amdmsm_ctx *ctx, int curve, const void *d_values, size_t m, size_t batch, size_t in_stride,
                                      size_t out_stride, int flags, const void *coset, int tile_log2, const amdmsm_opts *opts,
                                      void *d_out) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frdom_batch_plan b;
    frdom_params q;
    // the batch's own alignment and overlap rules stand in for those of one vector
    int rc = frdom_check(ctx, f, d_values, m, flags, coset, tile_log2, opts, d_out, false, b.p, q, batch != 0);
    if (!rc) rc = fr_check_batch(ctx, f, "m", m, batch, in_stride, out_stride, d_values, d_out, true);
    if (rc) return rc;
    FR_ENTER(ctx);
    if (!batch) return AMDMSM_OK;
    frdom_make_batch_plan(b.p, batch, b);
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, b.ws_bytes, {}, {}, [&](char *, char *ws) {
        return frdom_run_batch(ctx, f, st, b, q, (const uint32_t *)d_values, in_stride, (uint32_t *)d_out, out_stride, ws);
    });
}

int amdmsm_plan_fr_qap_witness_map(int curve, size_t m, size_t out[6]) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return AMDMSM_ERR_UNSUPPORTED;
    if (!out) return AMDMSM_ERR_BAD_ARG;
    frqap_call c;
    const int rc = frqap_check(nullptr, f, nullptr, 0, m, nullptr, nullptr, out, false, c);
    if (rc) return rc;
    const frdom &d = c.dp.d;
    out[0] = d.step ? AMDMSM_DOMAIN_STEP_RADIX2 : AMDMSM_DOMAIN_BASIC_RADIX2;
    out[1] = d.m;
    out[2] = d.B;
    out[3] = d.S;
    // without the partial sums of the applies, which belong to the handles
    out[4] = align_up(3 * m * c.rec, 256) + c.bp.ws_bytes + std::max<size_t>(c.div.ws_bytes, 256);
    out[5] = 2 * ((size_t)c.bp.bb.p.passes + (d.step ? (size_t)c.bp.bs.p.passes : 0));
    return AMDMSM_OK;
}

int amdmsm_fr_qap_witness_map_device(amdmsm_ctx *ctx, int curve, uint64_t mat_a, uint64_t mat_b, uint64_t mat_c, const void *d_z,
                                     size_t n_z, size_t m, const void *blind, const amdmsm_opts *opts, void *d_h) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frqap_call c;
    int rc = frqap_check(ctx, f, d_z, n_z, m, blind, opts, d_h, true, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    const uint64_t mats[3] = {mat_a, mat_b, mat_c};
    rc = frqap_handles(ctx, f, mats, n_z, m, c);
    if (rc) return rc;
    hipStream_t st = stream_of(ctx, opts);
    return fr_call(ctx, st, 0, c.ws_bytes, {}, {}, [&](char *, char *ws) {
        return frqap_run(ctx, f, st, c, (const uint32_t *)d_z, (uint32_t *)d_h, ws);
    });
}

int amdmsm_fr_qap_witness_map(amdmsm_ctx *ctx, int curve, uint64_t mat_a, uint64_t mat_b, uint64_t mat_c, const void *z, size_t n_z,
                              size_t m, const void *blind, const amdmsm_opts *opts, void *h) {
    const fr_vtable *f = find_frvt(curve);
    if (!f) return fail(ctx, AMDMSM_ERR_UNSUPPORTED, "unknown curve");
    CHECK_OPTS(ctx, opts);
    frqap_call c;
    int rc = frqap_check(ctx, f, z, n_z, m, blind, opts, h, false, c);
    if (rc) return rc;
    FR_ENTER(ctx);
    const uint64_t mats[3] = {mat_a, mat_b, mat_c};
    rc = frqap_handles(ctx, f, mats, n_z, m, c);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    // staged: z and h, in that order
    const size_t z_bytes = align_up((n_z ? n_z : 1) * c.rec, 256), h_bytes = align_up((m + 1) * c.rec, 256);
    return fr_call(ctx, st, z_bytes + h_bytes, c.ws_bytes, {{z, 0, n_z * c.rec}}, {{h, z_bytes, (m + 1) * c.rec}}, [&](char *vecs, char *ws) {
        return frqap_run(ctx, f, st, c, (const uint32_t *)vecs, (uint32_t *)(vecs + z_bytes), ws);
    });
}

}  // extern "C"
