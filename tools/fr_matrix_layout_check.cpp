// Stand-alone check of libff_amd/csrc/fr_matrix_layout.h, the host code that turns a CSR matrix into the resident form
// of amdmsm_fr_matrix_load: builds layouts for a handful of small matrices, walks them the way k_frm_apply does -- wave
// job by wave job, step by step, lane by lane, every array a heap block of its exact size -- over a small prime, and
// compares with the plain CSR sum; the transposition in front of amdmsm_fr_matrix_load_transposed likewise.  Meant for the host compiler's sanitizers (tests/test_fr_matrix_cpu.py):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I libff_amd/csrc tools/fr_matrix_layout_check.cpp -o check && ./check
// No HIP, no GPU.  Exit status 0 and "ok" when every matrix agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fr_matrix_layout.h"

using namespace amdmsm;

namespace {

constexpr uint64_t P = 65521;   // the field of the check

struct csr {
    size_t n_rows = 0, n_cols = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> cols;
    std::vector<uint64_t> coeffs;
};

uint64_t rng_state = 88172645463325252ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
uint64_t pick_coeff() {
    switch (rnd() % 8) {
    case 0: return 0;
    case 1: case 2: case 3: return 1;
    case 4: return P - 1;
    case 5: return 2;
    default: return rnd() % P;
    }
}

template <class T>
std::unique_ptr<T[]> exact_copy(const std::vector<T> &v) {   // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

csr make(size_t n_cols, const std::vector<size_t> &lens, bool nonzero = false) {
    csr m;
    m.n_rows = lens.size();
    m.n_cols = n_cols;
    m.offsets.push_back(0);
    for (size_t len : lens) {
        for (size_t e = 0; e < len; ++e) {
            m.cols.push_back((uint32_t)(rnd() % n_cols));
            uint64_t c = pick_coeff();
            if (nonzero && c == 0) c = 3;
            m.coeffs.push_back(c);
        }
        m.offsets.push_back(m.cols.size());
    }
    return m;
}

// the transpose through frm_transpose, its arrays read from heap blocks of exact size; 1 where it is not the transpose
int transposed(const char *name, const csr &m, csr &t) {
    auto offsets = exact_copy(m.offsets), coeffs = exact_copy(m.coeffs);
    auto cols = exact_copy(m.cols);
    frm_transposed tr;
    frm_transpose(m.n_rows, m.n_cols, m.n_rows ? offsets.get() : nullptr, cols.get(), tr);
    t = csr();
    t.n_rows = m.n_cols;
    t.n_cols = m.n_rows;
    t.offsets = tr.offsets;
    t.cols = tr.rows;
    for (uint32_t k : tr.src) t.coeffs.push_back(coeffs[k]);
    // every entry of M once, under its column, rows ascending and the entries of one row in the order given
    int wrong = t.offsets.size() != m.n_cols + 1 || t.cols.size() != m.cols.size() || tr.src.size() != m.cols.size();
    std::vector<char> seen(m.cols.size(), 0);
    for (size_t c = 0; !wrong && c < m.n_cols; ++c)
        for (uint64_t k = t.offsets[c]; k < t.offsets[c + 1]; ++k) {
            const uint32_t src = tr.src[k], row = tr.rows[k];
            wrong += src >= m.cols.size() || seen[src]++ || m.cols[src] != c || src < m.offsets[row] || src >= m.offsets[row + 1];
            if (k > t.offsets[c]) wrong += tr.src[k - 1] >= src;
        }
    if (wrong) printf("%s: not the transpose\n", name);
    return wrong ? 1 : 0;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

int check(const char *name, const csr &m, uint32_t t_wave, uint32_t t_split, size_t n_out) {
    std::string err;
    if (frm_validate(m.n_rows, m.n_cols, m.n_rows ? m.offsets.data() : nullptr, m.cols.data(), true, err)) {
        printf("%s: validation: %s\n", name, err.c_str());
        return 1;
    }
    frm_layout L;
    uint64_t bad = 0;
    const auto cls_of = [&](uint64_t k) -> uint32_t {
        const uint64_t c = m.coeffs[k];
        return c >= P ? FRM_BAD : c == 1 ? FRM_PLUS : c == P - 1 ? FRM_MINUS : c == 0 ? FRM_ZERO : FRM_GEN;
    };
    if (!frm_build(m.n_rows, m.offsets.data(), m.cols.data(), cls_of, t_wave, t_split, L, bad)) {
        printf("%s: entry %llu refused\n", name, (unsigned long long)bad);
        return 1;
    }
    // what the device holds, and the vectors
    std::vector<uint64_t> coef_v;
    for (uint64_t k : L.gen_src) coef_v.push_back(m.coeffs[k]);
    std::vector<uint64_t> x_v(m.n_cols), out_v(n_out, 0xdeadbeef), part_v(L.n_partials, 0xdeadbeef);
    for (auto &v : x_v) v = rnd() % P;
    auto words = exact(L.words);
    auto coef = exact(coef_v);
    auto desc = exact(L.desc);
    auto lane_rows = exact(L.lane_rows);
    auto comb = exact(L.comb);
    auto x = exact(x_v);
    auto out = exact(out_v);
    auto part = exact(part_v);

    for (size_t wv = 0; wv < L.desc.size(); ++wv) {
        const frm_desc d = desc[wv];
        const uint32_t mode = d.dest >> FRM_MODE_SHIFT, dest = d.dest & FRM_DEST_MASK;
        uint64_t sum[FRM_LANES] = {};
        uint32_t rank0 = d.gen_base;
        for (uint32_t j = 0; j < d.steps; ++j) {
            uint32_t below = 0;
            for (uint32_t lane = 0; lane < FRM_LANES; ++lane) {
                const uint32_t w = words[((size_t)d.base64 + j) * FRM_LANES + lane];
                const uint32_t cls = w >> FRM_COL_BITS;
                if (cls == FRM_PAD) continue;
                const uint64_t xv = x[w & FRM_COL_MASK];
                if (cls == FRM_GEN) sum[lane] = (sum[lane] + coef[rank0 + below++] * xv) % P;
                else sum[lane] = (sum[lane] + (cls == FRM_MINUS ? P - xv : xv)) % P;
            }
            rank0 += below;
        }
        if (mode == FRM_MODE_LANES) {
            for (uint32_t lane = 0; lane < FRM_LANES; ++lane) {
                const uint32_t row = lane_rows[(size_t)dest * FRM_LANES + lane];
                if (row != FRM_NO_ROW) out[row] = sum[lane];
            }
        } else {
            uint64_t s = 0;
            for (uint32_t lane = 0; lane < FRM_LANES; ++lane) s = (s + sum[lane]) % P;
            (mode == FRM_MODE_PART ? part : out)[dest] = s;
        }
    }
    for (size_t i = m.n_rows; i < n_out; ++i) out[i] = 0;
    for (size_t c = 0; c < L.comb.size(); ++c) {
        uint64_t s = 0;
        for (uint32_t p = 0; p < comb[c].count; ++p) s = (s + part[comb[c].first + p]) % P;
        out[comb[c].row] = s;
    }

    int wrong = 0;
    uint64_t kept = 0;
    for (size_t i = 0; i < m.n_rows; ++i) {
        uint64_t s = 0;
        for (uint64_t k = m.offsets[i]; k < m.offsets[i + 1]; ++k) {
            s = (s + m.coeffs[k] * x_v[m.cols[k]]) % P;
            kept += m.coeffs[k] != 0;
        }
        if (out[i] != s && !wrong++) printf("%s: row %zu: %llu, want %llu\n", name, i, (unsigned long long)out[i], (unsigned long long)s);
    }
    for (size_t i = m.n_rows; i < n_out; ++i) wrong += out[i] != 0;
    // the counts the plan entry reports
    if (L.rows_lane + L.rows_wave + L.rows_split != m.n_rows || L.cnt[FRM_GEN] + L.cnt[FRM_PLUS] + L.cnt[FRM_MINUS] != kept ||
        L.cnt[FRM_GEN] != L.gen_src.size() || L.words.size() % FRM_LANES || L.lane_rows.size() % FRM_LANES ||
        L.comb.size() != L.rows_split) {
        printf("%s: counts disagree\n", name);
        ++wrong;
    }
    printf("%-28s rows %zu nnz %llu jobs %zu words %zu partials %u: %s\n", name, m.n_rows, (unsigned long long)L.nnz, L.desc.size(),
           L.words.size(), L.n_partials, wrong ? "WRONG" : "ok");
    return wrong ? 1 : 0;
}

}  // namespace

int main() {
    int bad = 0;
    uint32_t tw, ts;
    frm_thresholds(0, 0, tw, ts);
    bad += check("no rows", make(1, {}), 0, 0, 0);
    bad += check("no rows, a tail", make(1, {}), 0, 0, 5);
    bad += check("empty rows", make(3, std::vector<size_t>(130, 0)), 0, 0, 130);
    bad += check("one entry", make(1, {1}), 0, 0, 1);
    bad += check("rows 0..3", make(7, {0, 1, 2, 3, 3, 2, 1, 0, 2}), 0, 0, 16);
    {   // every class edge at the default thresholds; non-zero coefficients, so that the lengths are what they say
        std::vector<size_t> lens = {tw - 1, tw, tw + 1, 63, 64, 65, 127, 128, 129, ts - 1, ts, ts + 1, 2 * ts, 2 * ts + 1, 0, 5};
        bad += check("class edges", make(200, lens, true), 0, 0, lens.size() + 3);
        bad += check("class edges, zeros dropped", make(200, lens), 0, 0, lens.size());
    }
    {   // small thresholds: the same edges with more rows per class, and 63 / 64 / 65 rows to a block
        for (size_t rows : {63, 64, 65, 129}) {
            std::vector<size_t> lens;
            for (size_t i = 0; i < rows; ++i) lens.push_back(rnd() % 4);
            bad += check("lane blocks", make(50, lens), 4, 64, rows);
        }
        std::vector<size_t> lens;
        for (size_t i = 0; i < 300; ++i) lens.push_back(rnd() % 10 == 0 ? 60 + rnd() % 200 : rnd() % 9);
        bad += check("mixed, t_wave 4 t_split 64", make(97, lens), 4, 64, 512);
        bad += check("mixed, t_wave 1", make(97, lens), 1, 64, 300);
    }
    bad += check("one long row", make(11, {70000}), 0, 0, 1);
    {   // amdmsm_fr_matrix_load_transposed: the transpose, and its layout walked like any other
        std::vector<size_t> lens;
        for (size_t i = 0; i < 3000; ++i) lens.push_back(1 + rnd() % 4);
        csr wide = make(40, lens), t;
        for (size_t i = 0; i < wide.n_rows; ++i) wide.cols[wide.offsets[i]] = 0;   // one column in every row
        bad += transposed("transposed, a full column", wide, t) || check("transposed, a full column", t, 4, 256, 64);
        bad += transposed("transposed, rows 0..3", make(7, {0, 1, 2, 3, 3, 2, 1, 0, 2}), t) || check("transposed, rows 0..3", t, 0, 0, 7);
        bad += transposed("transposed, no rows", make(5, {}), t) || check("transposed, no rows", t, 0, 0, 5);
        csr none = make(1, {0, 0, 0});
        none.n_cols = 0;
        bad += transposed("transposed, no columns", none, t) || check("transposed, no columns", t, 0, 0, 0);
    }
    {   // the refusals of the index rules
        std::string err;
        const uint64_t off_bad0[] = {1, 2}, off_dec[] = {0, 2, 1}, off_ok[] = {0, 1};
        const uint32_t c[] = {0, 5};
        int r = 0;
        r += frm_validate(1, 8, off_bad0, c, true, err) != 1;
        r += frm_validate(2, 8, off_dec, c, true, err) != 1;
        r += frm_validate(1, 8, off_ok, c + 1, true, err) == 0 ? 0 : 1;
        r += frm_validate(1, 5, off_ok, c + 1, true, err) != 1;
        r += frm_validate(1, 8, nullptr, c, true, err) != 1;
        r += frm_validate(1, 8, off_ok, nullptr, true, err) != 1;
        r += frm_validate(1, 8, off_ok, c, false, err) != 1;
        r += frm_validate(FRM_MAX_DIM + 1, 8, off_ok, c, true, err) != 2;
        r += frm_validate(1, FRM_MAX_DIM + 1, off_ok, c, true, err) != 2;
        const uint64_t off_big[] = {0, FRM_MAX_NNZ + 1};
        r += frm_validate(1, 8, off_big, c, true, err) != 2;
        printf("%-28s %s\n", "refusals", r ? "WRONG" : "ok");
        bad += r;
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
