// Scans and batch inversion over Fr vectors (amdmsm_fr_scan, amdmsm_fr_batch_invert): the tile counts, the spine's steps,
// the workspace offsets and every index the three kernels of fr_scan.inc form.  Pure index arithmetic -- no HIP, no field
// arithmetic -- shared by the kernels, by engine.cpp and by the stand-alone checker tools/fr_scan_layout_check.cpp, which
// walks the same functions against heap blocks of exact size under the host compiler's sanitizers.  DESIGN section 20.
//
// A vector of n records is cut into tiles of 2^tile_log2 positions; a tile is one workgroup of FRS_LANES lanes with
// 2^(tile_log2 - 8) consecutive positions each.  Position p is record p of the vector, or record n - 1 - p of a reverse
// scan: the kernels work on positions and never know the direction otherwise.  The tiles' aggregates -- one record A and
// one record B each -- lie in the workspace, where one workgroup (the spine) walks them a step at a time -- FRS_LANES
// lanes with frs_spine_per_lane consecutive aggregates each -- and leaves each tile's incoming value.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FRS_HD __host__ __device__ inline
#else
#define FRS_HD inline
#endif

namespace amdmsm {

constexpr uint32_t FRS_LANES = 256;
constexpr int FRS_LANES_LOG2 = 8;
constexpr int FRS_TILE_MIN = 8, FRS_TILE_MAX = 10, FRS_TILE_DEFAULT = 10;   // records of a tile (log2); default: profiles/fr_scan.txt
constexpr uint32_t FRS_PER_LANE_MAX = 1u << (FRS_TILE_MAX - FRS_LANES_LOG2);
// Tile aggregates a lane of the spine takes per step.  A step costs the block scan's dozen dependent products whatever
// it holds and a lane's aggregates one or two each, so a lane takes more of them the more tiles there are: the smallest
// power of two that brings the tiles into 64 lanes' reach, at most 1, 4, 16 for tiles of 2^8, 2^9, 2^10 records.  The
// smallest tile keeps one, so that 2^16 records already make a second step.
FRS_HD uint32_t frs_spine_per_lane(int tile_log2, size_t tiles) {
    const uint32_t most = 1u << (2 * (tile_log2 - FRS_TILE_MIN));
    uint32_t g = 1;
    while (g < most && (size_t)64 * g < tiles) g <<= 1;
    return g;
}
constexpr size_t FRS_MAX_N = (size_t)1 << 28;
// slots of the 2^10-record LDS tile the block scan uses once the tile's records are in registers
constexpr uint32_t FRS_SLOT_A = 0, FRS_SLOT_B = FRS_LANES, FRS_SLOT_TOTAL = 2 * FRS_LANES, FRS_SLOT_AUX = 2 * FRS_LANES + 2;

struct frs_layout {
    int tile_log2 = 0;
    uint32_t tile = 0, per_lane = 0;
    uint32_t spine_step = 0;              // tile aggregates of one spine step
    size_t tiles = 0, spine_steps = 0;
    size_t off_a = 0, off_b = 0, off_in = 0, off_cnt = 0, ws_bytes = 0;   // workspace: aggregates A, B, incoming values, zero counts
    int launches = 0;
};

FRS_HD size_t frs_align(size_t x) { return (x + 255) / 256 * 256; }

// tile_log2: 0 = the default.  naive: the one-lane path -- no tiles; an inversion keeps its n running products in the workspace
inline bool frs_make_layout(size_t n, int tile_log2, size_t rec_bytes, bool invert, bool naive, frs_layout &L) {
    if (tile_log2 && (tile_log2 < FRS_TILE_MIN || tile_log2 > FRS_TILE_MAX)) return false;
    L = frs_layout();
    L.tile_log2 = tile_log2 ? tile_log2 : FRS_TILE_DEFAULT;
    L.tile = 1u << L.tile_log2;
    L.per_lane = L.tile / FRS_LANES;
    L.tiles = (n + L.tile - 1) >> L.tile_log2;
    L.spine_step = FRS_LANES * frs_spine_per_lane(L.tile_log2, L.tiles);
    L.spine_steps = (L.tiles + L.spine_step - 1) / L.spine_step;
    if (naive) {
        L.launches = 1;
        L.ws_bytes = frs_align((invert ? (n ? n : 1) : 1) * rec_bytes);
        return true;
    }
    const size_t vec = frs_align((L.tiles ? L.tiles : 1) * rec_bytes);
    L.off_a = 0;
    L.off_b = vec;
    L.off_in = 2 * vec;
    L.off_cnt = 3 * vec;
    L.ws_bytes = L.off_cnt + frs_align((L.tiles ? L.tiles : 1) * sizeof(uint32_t));
    L.launches = n ? 3 : 1;   // reduce, spine, apply; the spine alone writes the total of an empty vector
    return true;
}

// ---- what the kernels index with -------------------------------------------------------------------------------------
// first position of a tile; position e of a tile while it is staged (e < tile); the positions of a lane
FRS_HD size_t frs_tile_base(uint32_t tile_index, int tile_log2) { return (size_t)tile_index << tile_log2; }
FRS_HD uint32_t frs_lane_slot(uint32_t lane, uint32_t k, int tile_log2) { return (lane << (tile_log2 - FRS_LANES_LOG2)) + k; }
// the record of the caller's vectors behind position p < n
FRS_HD size_t frs_record(size_t n, bool reverse, size_t p) { return reverse ? n - 1 - p : p; }
// the g-th aggregate (g < per_lane) of lane l in spine step s; backwards: the second sweep of an inversion, from the last
// tile down.  At or above `tiles`: none (the identity)
FRS_HD size_t frs_spine_tile(size_t tiles, uint32_t per_lane, size_t step, uint32_t lane, uint32_t g, bool backwards) {
    const size_t r = (step * FRS_LANES + lane) * per_lane + g;
    if (r >= tiles) return tiles;
    return backwards ? tiles - 1 - r : r;
}
FRS_HD size_t frs_spine_steps(size_t tiles, uint32_t per_lane) {
    const size_t step = (size_t)FRS_LANES * per_lane;
    return (tiles + step - 1) / step;
}

}  // namespace amdmsm
