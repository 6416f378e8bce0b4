// CSR -> resident form of a sparse matrix over Fr (amdmsm_fr_matrix_load): validation, classification, binning, the
// row permutation and the offsets of the side arrays; and the CSR of the transpose (amdmsm_fr_matrix_load_transposed).  Pure index arithmetic on host arrays -- no HIP, no field
// arithmetic: the caller says what class a coefficient is -- so that the stand-alone checker tools/fr_matrix_layout_check.cpp
// builds the same layouts under the host compiler's sanitizers.  DESIGN section 19 describes the form.
//
// The resident form is a list of wave jobs (frm_desc), one per 64-lane wave of k_frm_apply, over one array of entry
// words, 64 per step: lane l of the wave reads word (base64 + j) * 64 + l in step j.  A word is a column (28 bits) and
// a class (4 bits).  Three kinds of job:
//   FRM_MODE_LANES  64 rows shorter than t_wave, one per lane, `steps` = the longest of them; lane l writes row
//                   lane_rows[dest * 64 + l] (FRM_NO_ROW: none).  The rows are taken in order of length, so the lanes
//                   of a wave finish together.
//   FRM_MODE_ROW    one row of t_wave .. t_split entries, entry e in step e / 64 at lane e % 64; the lanes' sums are
//                   combined and row `dest` is written.
//   FRM_MODE_PART   t_split entries (the last piece: the rest) of a longer row, as FRM_MODE_ROW, written to
//                   partial[dest]; frm_comb lists each such row's partials for the second step.
// Entries with coefficient 1 and r - 1 carry no coefficient; the general ones read record gen_base + (their rank among
// the job's general entries in word order) of the side array, which gen_src lists as positions of the caller's CSR.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace amdmsm {

constexpr uint32_t FRM_LANES = 64;
constexpr int FRM_COL_BITS = 28;
constexpr uint32_t FRM_COL_MASK = (1u << FRM_COL_BITS) - 1;
// classes of an entry word (its top four bits); FRM_ZERO and FRM_BAD are what a classifier may also answer
enum : uint32_t { FRM_GEN = 0, FRM_PLUS = 1, FRM_MINUS = 2, FRM_PAD = 3, FRM_ZERO = 4, FRM_BAD = 5 };
enum : uint32_t { FRM_MODE_LANES = 0, FRM_MODE_ROW = 1, FRM_MODE_PART = 2 };
constexpr int FRM_MODE_SHIFT = 30;
constexpr uint32_t FRM_DEST_MASK = (1u << FRM_MODE_SHIFT) - 1;
constexpr uint32_t FRM_NO_ROW = 0xffffffffu;
constexpr uint64_t FRM_NO_ENTRY = ~(uint64_t)0;
constexpr size_t FRM_MAX_DIM = (size_t)1 << 28;   // rows, columns: a column fits FRM_COL_BITS
constexpr size_t FRM_MAX_NNZ = (size_t)1 << 31;
constexpr uint32_t FRM_T_WAVE_DEFAULT = 32, FRM_T_SPLIT_DEFAULT = 1024;   // measured: profiles/fr_matrix.txt

struct frm_desc {
    uint32_t base64;     // first step of the job, in units of 64 words
    uint32_t steps;
    uint32_t gen_base;   // rank of the job's first general entry in the side array
    uint32_t dest;       // mode << FRM_MODE_SHIFT | block of lane_rows / row / partial
};
struct frm_comb {
    uint32_t row, first, count;   // out[row] = partial[first] + .. + partial[first + count - 1]
};

struct frm_layout {
    uint64_t nnz = 0, cnt[5] = {};                  // entries given; per class (FRM_GEN, FRM_PLUS, FRM_MINUS, -, FRM_ZERO)
    uint64_t rows_lane = 0, rows_wave = 0, rows_split = 0, longest = 0;
    uint32_t t_wave = 0, t_split = 0;
    std::vector<uint32_t> words;
    std::vector<uint64_t> gen_src;
    std::vector<frm_desc> desc;
    std::vector<uint32_t> lane_rows;
    std::vector<frm_comb> comb;
    uint32_t n_partials = 0;
};

// The thresholds a layout is built with: rows below t_wave go one to a lane, rows above t_split are cut into pieces of
// t_split entries; t_split is a whole number of steps and at least t_wave.
inline void frm_thresholds(uint32_t want_wave, uint32_t want_split, uint32_t &t_wave, uint32_t &t_split) {
    t_wave = want_wave ? want_wave : FRM_T_WAVE_DEFAULT;
    if (t_wave > 4096) t_wave = 4096;
    t_split = want_split ? want_split : FRM_T_SPLIT_DEFAULT;
    if (t_split > (1u << 20)) t_split = 1u << 20;
    t_split = (t_split + FRM_LANES - 1) / FRM_LANES * FRM_LANES;
    while (t_split < t_wave) t_split += FRM_LANES;
}

// The index rules of the load: 0, or the error code class 1 = bad argument, 2 = too large, with the row or entry named.
inline int frm_validate(size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols, bool have_coeffs,
                        std::string &err) {
    if (n_rows > FRM_MAX_DIM) return err = "n_rows = " + std::to_string(n_rows) + ": at most 2^28 rows", 2;
    if (n_cols > FRM_MAX_DIM) return err = "n_cols = " + std::to_string(n_cols) + ": at most 2^28 columns", 2;
    if (!n_rows) return 0;
    if (!offsets) return err = "offsets: null pointer", 1;
    if (offsets[0] != 0) return err = "offsets[0] = " + std::to_string(offsets[0]) + ", not 0", 1;
    for (size_t i = 0; i < n_rows; ++i)
        if (offsets[i + 1] < offsets[i])
            return err = "row " + std::to_string(i) + ": offsets decrease (" + std::to_string(offsets[i]) + " -> " +
                         std::to_string(offsets[i + 1]) + ")", 1;
    const uint64_t nnz = offsets[n_rows];
    if (nnz > FRM_MAX_NNZ) return err = "nnz = " + std::to_string(nnz) + ": at most 2^31 entries", 2;
    if (nnz && !cols) return err = "cols: null pointer", 1;
    if (nnz && !have_coeffs) return err = "coeffs: null pointer", 1;
    for (uint64_t k = 0; k < nnz; ++k)
        if (cols[k] >= n_cols)
            return err = "entry " + std::to_string(k) + ": column " + std::to_string(cols[k]) + " >= n_cols = " +
                         std::to_string(n_cols), 1;
    return 0;
}

// The CSR of the transpose of a validated matrix M (amdmsm_fr_matrix_load_transposed), by a stable counting sort on the
// column: n_cols rows whose entries go in ascending row of M, those of one row of M in the order given.  src[k]: the
// entry of M behind entry k of the transpose -- the coefficients stay where the caller has them.
struct frm_transposed {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> rows, src;
};
inline void frm_transpose(size_t n_rows, size_t n_cols, const uint64_t *offsets, const uint32_t *cols, frm_transposed &t) {
    const uint64_t nnz = n_rows ? offsets[n_rows] : 0;
    t.offsets.assign(n_cols + 1, 0);
    for (uint64_t k = 0; k < nnz; ++k) ++t.offsets[(size_t)cols[k] + 1];
    for (size_t c = 0; c < n_cols; ++c) t.offsets[c + 1] += t.offsets[c];
    t.rows.resize(nnz);
    t.src.resize(nnz);
    std::vector<uint64_t> at(t.offsets.begin(), t.offsets.end() - 1);
    for (size_t i = 0; i < n_rows; ++i)
        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) {
            const uint64_t p = at[cols[k]]++;
            t.rows[p] = (uint32_t)i;
            t.src[p] = (uint32_t)k;   // nnz <= 2^31
        }
}

// The layout of a validated matrix.  cls_of(k): the class of the caller's entry k -- FRM_GEN, FRM_PLUS, FRM_MINUS,
// FRM_ZERO, or FRM_BAD for a coefficient that is no field element, which ends the build: false, with `bad` the entry.
template <class ClsOf>
bool frm_build(size_t n_rows, const uint64_t *offsets, const uint32_t *cols, ClsOf &&cls_of, uint32_t want_wave,
               uint32_t want_split, frm_layout &L, uint64_t &bad) {
    L = frm_layout();
    frm_thresholds(want_wave, want_split, L.t_wave, L.t_split);
    L.nnz = n_rows ? offsets[n_rows] : 0;
    // one pass over the entries: classes, and the kept (non-zero) length of every row
    std::vector<uint8_t> cls(L.nnz);
    std::vector<uint32_t> len(n_rows, 0);
    for (size_t i = 0; i < n_rows; ++i) {
        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) {
            const uint32_t c = cls_of(k);
            if (c != FRM_GEN && c != FRM_PLUS && c != FRM_MINUS && c != FRM_ZERO) {
                bad = k;
                return false;
            }
            cls[k] = (uint8_t)c;
            ++L.cnt[c];
            if (c != FRM_ZERO) ++len[i];
        }
        if (len[i] > L.longest) L.longest = len[i];
    }
    // rows below t_wave in order of length, equal lengths in row order (counting sort)
    std::vector<uint64_t> start((size_t)L.t_wave + 1, 0);
    for (size_t i = 0; i < n_rows; ++i)
        if (len[i] < L.t_wave) ++start[len[i] + 1];
    for (uint32_t l = 0; l < L.t_wave; ++l) start[l + 1] += start[l];
    L.rows_lane = start[L.t_wave];
    std::vector<uint32_t> order(L.rows_lane);
    for (size_t i = 0; i < n_rows; ++i)
        if (len[i] < L.t_wave) order[start[len[i]]++] = (uint32_t)i;

    // A job from the CSR positions of its words (src, FRM_NO_ENTRY: padding): the words, and the general entries in word
    // order -- the order in which the kernel ranks them -- appended to the side array's source list.
    uint64_t steps_total = 0;
    std::vector<uint64_t> src;
    const auto emit_job = [&](uint32_t steps, uint32_t mode, uint32_t dest) {
        const frm_desc d = {(uint32_t)steps_total, steps, (uint32_t)L.gen_src.size(), (mode << FRM_MODE_SHIFT) | dest};
        L.desc.push_back(d);
        for (uint64_t w = 0; w < (uint64_t)steps * FRM_LANES; ++w) {
            const uint64_t k = src[w];
            if (k == FRM_NO_ENTRY) {
                L.words.push_back((uint32_t)FRM_PAD << FRM_COL_BITS);
                continue;
            }
            L.words.push_back(cols[k] | ((uint32_t)cls[k] << FRM_COL_BITS));
            if (cls[k] == FRM_GEN) L.gen_src.push_back(k);
        }
        steps_total += steps;
    };

    for (uint64_t b = 0; b < L.rows_lane; b += FRM_LANES) {
        const uint64_t rows = L.rows_lane - b < FRM_LANES ? L.rows_lane - b : FRM_LANES;
        const uint32_t steps = len[order[b + rows - 1]];   // the longest of the block is its last
        src.assign((size_t)steps * FRM_LANES, FRM_NO_ENTRY);
        const uint32_t block = (uint32_t)(L.lane_rows.size() / FRM_LANES);
        for (uint64_t l = 0; l < FRM_LANES; ++l) {
            const uint32_t row = l < rows ? order[b + l] : FRM_NO_ROW;
            L.lane_rows.push_back(row);
            if (row == FRM_NO_ROW) continue;
            uint64_t j = 0;
            for (uint64_t k = offsets[row]; k < offsets[row + 1]; ++k)
                if (cls[k] != FRM_ZERO) src[j++ * FRM_LANES + l] = k;
        }
        emit_job(steps, FRM_MODE_LANES, block);
    }
    std::vector<uint64_t> kept;
    for (size_t i = 0; i < n_rows; ++i) {
        if (len[i] < L.t_wave) continue;
        kept.clear();
        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k)
            if (cls[k] != FRM_ZERO) kept.push_back(k);
        const bool split = kept.size() > L.t_split;
        if (split) {
            const frm_comb c = {(uint32_t)i, L.n_partials, (uint32_t)((kept.size() + L.t_split - 1) / L.t_split)};
            L.comb.push_back(c);
            ++L.rows_split;
        } else {
            ++L.rows_wave;
        }
        for (uint64_t at = 0; at < kept.size(); at += L.t_split) {
            const uint64_t take = kept.size() - at < L.t_split ? kept.size() - at : L.t_split;
            const uint32_t steps = (uint32_t)((take + FRM_LANES - 1) / FRM_LANES);
            src.assign((size_t)steps * FRM_LANES, FRM_NO_ENTRY);
            for (uint64_t e = 0; e < take; ++e) src[e] = kept[at + e];
            if (split) emit_job(steps, FRM_MODE_PART, L.n_partials++);
            else emit_job(steps, FRM_MODE_ROW, (uint32_t)i);
        }
    }
    return true;
}

}  // namespace amdmsm
