// Stand-alone check of the index arithmetic of the Fr scans (libff_amd/csrc/fr_scan_layout.h): walks every index the
// three kernels of fr_scan.inc form -- the records a tile stages, the slots of its lanes, the aggregates and incoming
// values in the workspace, the tiles of every spine step in both sweeps -- for n around every edge and every tile size,
// against heap blocks of exact size.  Built with the host compiler and its sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I libff_amd/csrc tools/fr_scan_layout_check.cpp -o check && ./check
// Prints "ok" and exits 0, or names the first rule that fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "fr_scan_layout.h"

using namespace amdmsm;

static long long g_cases = 0;
#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::printf("FAILED %s:%d: %s (n = %zu, tile_log2 = %d)\n", __FILE__, __LINE__, #cond, n, tl); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

constexpr uint32_t LDS_RECORDS = 1024;   // the LDS tile of the scalar-field unit (FR_LDS_LOG2)

// one call: n records of rec bytes each, the given tile, scan or inversion, forward or reverse
static void walk(size_t n, int tl, size_t rec, bool invert, bool reverse) {
    frs_layout L;
    REQUIRE(frs_make_layout(n, tl, rec, invert, false, L));
    REQUIRE(L.tile == 1u << L.tile_log2 && L.per_lane * FRS_LANES == L.tile && L.per_lane <= FRS_PER_LANE_MAX);
    REQUIRE(L.tiles * L.tile >= n && (L.tiles == 0 || (L.tiles - 1) * (size_t)L.tile < n));
    const uint32_t G = frs_spine_per_lane(L.tile_log2, L.tiles);
    REQUIRE(L.spine_step == FRS_LANES * G && L.spine_steps == frs_spine_steps(L.tiles, G));
    REQUIRE(L.spine_steps * L.spine_step >= L.tiles && (L.spine_steps == 0 || (L.spine_steps - 1) * (size_t)L.spine_step < L.tiles));
    REQUIRE(L.launches == (n ? 3 : 1));
    // the workspace's four arrays lie apart and inside it
    REQUIRE(L.off_a + L.tiles * rec <= L.off_b && L.off_b + L.tiles * rec <= L.off_in && L.off_in + L.tiles * rec <= L.off_cnt);
    REQUIRE(L.off_cnt + L.tiles * 4 <= L.ws_bytes);
    // blocks of exact size: a byte stands for a word of a record
    std::unique_ptr<uint8_t[]> in(new uint8_t[n * rec]()), out(new uint8_t[n * rec]()), ws(new uint8_t[L.ws_bytes]());
    std::unique_ptr<uint8_t[]> lds(new uint8_t[LDS_RECORDS]());
    const int tlog = L.tile_log2;
    for (int pass = 0; pass < 2; ++pass) {   // reduce, apply
        for (uint32_t t = 0; t < L.tiles; ++t) {
            const size_t base = frs_tile_base(t, tlog);
            std::memset(lds.get(), 0, LDS_RECORDS);
            for (uint32_t e = 0; e < L.tile; ++e) {   // staging: every position of the tile once
                const size_t p = base + e;
                if (p < n) {
                    const size_t i = frs_record(n, reverse, p);
                    REQUIRE(i < n);
                    in[i * rec + rec - 1] += 1;
                }
                lds[e] += 1;
            }
            for (uint32_t lane = 0; lane < FRS_LANES; ++lane)   // the lanes take every staged position once
                for (uint32_t k = 0; k < L.per_lane; ++k) {
                    const uint32_t slot = frs_lane_slot(lane, k, tlog);
                    REQUIRE(slot < L.tile && lds[slot] == 1);
                    lds[slot] = 2;
                }
            for (uint32_t e = 0; e < L.tile; ++e) REQUIRE(lds[e] == 2);
            // the block scan's slots
            REQUIRE(FRS_SLOT_A + FRS_LANES <= FRS_SLOT_B && FRS_SLOT_B + FRS_LANES <= FRS_SLOT_TOTAL && FRS_SLOT_TOTAL + 2 <= FRS_SLOT_AUX);
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t q = 0; q < 4; ++q) lds[FRS_SLOT_B + 4 * lane + q] = 3;
            lds[FRS_SLOT_TOTAL + 1] = lds[FRS_SLOT_AUX] = 3;
            if (pass == 0) {
                ws[L.off_a + t * rec + rec - 1] += 1;
                ws[L.off_b + t * rec + rec - 1] += 1;
                ws[L.off_cnt + t * 4 + 3] += 1;
            } else {
                REQUIRE(ws[L.off_in + t * rec + rec - 1] == (invert ? 2 : 1));   // the spine has left the tile its value
                for (uint32_t e = 0; e < L.tile; ++e) {
                    const size_t p = base + e;
                    if (p < n) out[frs_record(n, reverse, p) * rec] += 1;
                }
            }
        }
        if (pass) break;
        // the spine: every aggregate once per sweep, a lane beyond the tiles none
        for (int sweep = 0; sweep < (invert ? 2 : 1); ++sweep) {
            std::set<size_t> seen;
            for (size_t s = 0; s < L.spine_steps; ++s)
                for (uint32_t lane = 0; lane < FRS_LANES; ++lane) {
                    bool ended = false;   // a lane's aggregates are consecutive: once one is missing the rest are
                    for (uint32_t g = 0; g < G; ++g) {
                        const size_t t = frs_spine_tile(L.tiles, G, s, lane, g, sweep == 1);
                        REQUIRE(t <= L.tiles);
                        if (t == L.tiles) {
                            ended = true;
                            continue;
                        }
                        REQUIRE(!ended && seen.insert(t).second);
                        REQUIRE(ws[L.off_a + t * rec + rec - 1] == 1 && ws[L.off_b + t * rec + rec - 1] == 1 && ws[L.off_cnt + t * 4 + 3] == 1);
                        ws[L.off_in + t * rec + rec - 1] += 1;
                    }
                }
            REQUIRE(seen.size() == L.tiles);
            // a backwards sweep meets the tiles from the last one down
            if (sweep == 1 && L.tiles) REQUIRE(frs_spine_tile(L.tiles, G, 0, 0, 0, true) == L.tiles - 1);
        }
    }
    for (size_t i = 0; i < n; ++i) REQUIRE(in[i * rec + rec - 1] == 2 && out[i * rec] == 1);   // read by reduce and apply, written once
    ++g_cases;
}

// the spine alone over `tiles` aggregates of a tile size: every aggregate once per sweep, in a workspace of exact size
static void walk_spine(size_t tiles, int tl, size_t rec) {
    const size_t n = tiles << tl;
    frs_layout L;
    REQUIRE(frs_make_layout(n, tl, rec, true, false, L) && L.tiles == tiles);
    const uint32_t G = frs_spine_per_lane(L.tile_log2, L.tiles);
    std::unique_ptr<uint8_t[]> ws(new uint8_t[L.ws_bytes]());
    for (int sweep = 0; sweep < 2; ++sweep)
        for (size_t s = 0; s < L.spine_steps; ++s)
            for (uint32_t lane = 0; lane < FRS_LANES; ++lane)
                for (uint32_t g = 0; g < G; ++g) {
                    const size_t t = frs_spine_tile(L.tiles, G, s, lane, g, sweep == 1);
                    REQUIRE(t <= L.tiles);
                    if (t == L.tiles) continue;
                    ws[L.off_a + t * rec + rec - 1] += 1;
                    ws[L.off_b + t * rec + rec - 1] += 1;
                    ws[L.off_in + t * rec + rec - 1] += 1;
                    ws[L.off_cnt + t * 4 + 3] += 1;
                }
    for (size_t t = 0; t < tiles; ++t) REQUIRE(ws[L.off_a + t * rec + rec - 1] == 2 && ws[L.off_in + t * rec + rec - 1] == 2 && ws[L.off_cnt + t * 4 + 3] == 2);
    ++g_cases;
}

int main() {
    size_t n = 0;
    int tl = 0;
    // the naive path: one launch, an inversion keeps n running products
    {
        frs_layout L;
        REQUIRE(frs_make_layout(1000, 0, 32, true, true, L) && L.launches == 1 && L.ws_bytes >= 1000 * 32);
        REQUIRE(frs_make_layout(0, 0, 48, false, true, L) && L.launches == 1 && L.ws_bytes >= 48);
        REQUIRE(!frs_make_layout(10, FRS_TILE_MIN - 1, 32, false, false, L) && !frs_make_layout(10, FRS_TILE_MAX + 1, 32, false, false, L));
        REQUIRE(frs_make_layout(FRS_MAX_N, FRS_TILE_MIN, 48, true, false, L) && L.tiles == FRS_MAX_N >> FRS_TILE_MIN && L.tiles <= 0xffffffffu);
    }
    for (tl = 0; tl <= FRS_TILE_MAX; tl = tl ? tl + 1 : FRS_TILE_MIN) {
        const int tlog = tl ? tl : FRS_TILE_DEFAULT;
        const size_t T = (size_t)1 << tlog, S = (size_t)FRS_LANES << (2 * (tlog - FRS_TILE_MIN));   // the largest step of the tile
        std::vector<size_t> sizes = {0, 1, 2, 63, 64, 65, 255, 256, 257};
        for (size_t edge : {T, 2 * T, 3 * T + 5, 40 * T, S * T, 2 * S * T})
            for (size_t d : {(size_t)0, (size_t)1, (size_t)2})
                sizes.push_back(edge + d - 1);
        for (size_t v : sizes) {
            n = v;
            if (n > ((size_t)1 << 17) + 1) continue;   // whole calls up to the sizes the device tests use
            for (size_t rec : {(size_t)32, (size_t)40, (size_t)48})
                for (int invert = 0; invert < 2; ++invert)
                    for (int reverse = 0; reverse < (invert ? 1 : 2); ++reverse) walk(n, tl, rec, invert != 0, reverse != 0);
        }
        // the spine's steps at every tile size, around one step's and two steps' worth of tiles
        for (size_t tiles : {(size_t)1, (size_t)64, (size_t)65, (size_t)128, (size_t)129, (size_t)257, (size_t)1025, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S - 1})
            for (size_t rec : {(size_t)32, (size_t)48}) {
                n = tiles << tlog;
                walk_spine(tiles, tlog, rec);
            }
    }
    std::printf("%lld cases\nok\n", g_cases);
    return 0;
}
