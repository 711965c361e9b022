// ttm_band_policy.h - which cache policy (template parameter POL of k_band_forward / k_band_inverse_ring, csrc/ttm_band.hip) a
// launch of the long band kernels takes.  Plain C++, no HIP: the decision is a function of sizes alone, so a CPU program can
// include this file and print it (tests/band_policy_gate.cpp).
//
// The model (OPTLOG round 12): the Infinity Cache is write-back and write-allocate for plain accesses and is
// passed by for non-temporal ones.  map() followed by inverse_map() writes Z and reads it back one launch later; with plain
// accesses throughout, a line of Z is read again only after the rest of both launches' traffic - twice the size of Z - has gone
// through the cache, so at sizes where Z alone does not fit, nothing of Z is left.  POL = 1
// lets only the rows of pair slot 0 of every tile of Z allocate - the first BAND_POLICY_HALF_ROWS rows of a tile - and moves
// everything else (X, the other half of Z, X') with non-temporal accesses, so that half can stay on-die from the forward launch
// to the inverse.
#pragma once

#include <stdint.h>

// The Infinity Cache of the MI355X: 256 MiB, die-level.  A buffer stays resident only while it and every byte that allocates
// between two uses of one of its lines fit in about this much (MI355X microarchitecture guide, section "Infinity Cache (L3)").
constexpr int64_t TTM_LLC_BYTES = (int64_t)256 << 20;

constexpr int BAND_POLICY_TILE_ROWS = 4096;          // rows of a tile of the long kernels (BAND_NS * BAND_CT; ttm_band.hip asserts it)
constexpr int BAND_POLICY_HALF_ROWS = 2048;          // rows of pair slot 0 of a full tile (2 * BAND_CT)

// bits of the decision
constexpr int BAND_POLICY_FORWARD = 1;               // k_band_forward takes POL = 1
constexpr int BAND_POLICY_INVERSE = 2;               // k_band_inverse_ring takes POL = 1

// rows of a column that pair slot 0 covers when N rows are cut into chunks of `chunk_rows` (chunk_grid) and a chunk into tiles:
// min(BAND_POLICY_HALF_ROWS, rows of the tile) per tile
static inline int64_t band_policy_resident_rows(int64_t N, int64_t chunk_rows) {
    if (N <= 0 || chunk_rows <= 0) return 0;
    auto of_chunk = [](int64_t n) {
        const int64_t tail = n % BAND_POLICY_TILE_ROWS;
        return n / BAND_POLICY_TILE_ROWS * BAND_POLICY_HALF_ROWS + (tail < BAND_POLICY_HALF_ROWS ? tail : BAND_POLICY_HALF_ROWS);
    };
    const int64_t whole = N / chunk_rows;            // chunks of chunk_rows rows; the last chunk has the rest
    return whole * of_chunk(chunk_rows) + of_chunk(N - whole * chunk_rows);
}

// ---- the cut of N rows into one chunk per workgroup (the long kernels) ----
// today's cut: N / #CUs rows rounded up to whole 128-byte lines of a column, so that every wave's 1 KB accesses are
// line-aligned (a chunk that starts inside a line makes every wave's store touch nine lines, two of them partially: the
// column stream then runs at 72 % of the copy rate: profiles/r03_*)
struct BandCut { int64_t rows, grid; bool full_tiles; };    // full_tiles: the rule below chose the cut
static inline int64_t band_policy_chunk_rows(int64_t N, int cus) {
    const int64_t rows = (N + cus - 1) / cus;
    return (rows + 31) / 32 * 32;
}
// option band_full_tiles (ttm_options.h): -1 auto, 0 off, 1 wherever whole tiles give every CU at most one chunk.
// k_band_forward and k_band_inverse_ring (both take THIS cut: the resident half of Z is defined by it) walk a full tile in
// a column loop of straight-line code with counted waits and a partial one in a masked loop that drains its loads at every
// loop-back.  Today's cut gives C5 at N = 1e6 on 256 CUs chunks of 3 936 rows: no workgroup has a full tile.  Chunks of one
// whole tile - ceil(N / 4096) workgroups, all but the last with a full tile - when that leaves at most 1 / 16 of the CUs
// without work: 1e6 rows -> 245 workgroups of 4 096 rows (OPTLOG round 15).
static inline BandCut band_policy_cut(int64_t N, int cus, int option) {
    if (cus < 1) cus = 1;
    const int64_t tiles = (N + BAND_POLICY_TILE_ROWS - 1) / BAND_POLICY_TILE_ROWS;
    const bool fits = N > 0 && tiles <= cus;
    if (option != 0 && fits && (option > 0 || tiles >= cus - cus / 16)) return {BAND_POLICY_TILE_ROWS, tiles, true};
    const int64_t rows = band_policy_chunk_rows(N, cus);
    return {rows, rows > 0 ? (N + rows - 1) / rows : 0, false};
}

// ---- Z through LDS, two columns deep (template parameter ZD of k_band_inverse_ring) ----
// bytes of LDS the two column buffers take: 2 columns x 16 waves x 2 pair slots x 1 KB
constexpr int64_t BAND_ZDMA_LDS_BYTES = 2 * (int64_t)BAND_POLICY_TILE_ROWS * 8;
// option band_zdma: -1 auto, 0 off, 1 wherever the kernel can run it.  ZD = 1 exists only beside POL = 1 and acts on full
// tiles only.  `ring_ok`: the ring keeps enough slots beside the buffers (band_ring_plan_with, ttm_band_image.h).
// Auto: off.  Measured at C5, N = 1e6, on the whole-tile cut (OPTLOG round 15, two GPUs): the inverse launch 0.1282 / 0.1259 ms
// against 0.1314 / 0.1269 ms - and 0.1274 / 0.1257 ms with ZD = 0 in the ring of 12 slots that ZD = 1 leaves: what little
// there is comes from the smaller ring (below), not from the path of z, and the step's ranges overlap.
static inline bool band_zdma_policy(int64_t N, BandCut cut, bool pol_inverse, bool ring_ok, int option) {
    if (option <= 0 || !pol_inverse || !ring_ok) return false;
    return N >= BAND_POLICY_TILE_ROWS && cut.rows >= BAND_POLICY_TILE_ROWS;             // (a full tile somewhere)
}

// ---- slots of a refilled ring (k_band_inverse_ring, G > 0) ----
// option band_ring_slots: -1 / 0 as many as fit (24 at C5), > 0 at most that many (whole groups, 3 G at least;
// band_ring_plan_with).  Every slot is filled in front of the first column - 6 KB each at C5, 150 KB per workgroup before the
// first row is looked up - while a step needs the images of the next 2 G steps only.  There is no automatic choice: 12 slots
// were faster than 24 in every comparison of OPTLOG round 15, but never by more than the two ranges added - not a gain by the
// log's rule.  The option stays as the instrument that tells ZD = 1 from the smaller ring it brings with it.

// option band_resident (ttm_options.h): -1 auto, 0 off, 1 forward only, 2 inverse only, 3 both - 1..3 whatever the size (tests,
// A/B runs).  Auto is both or none - either half alone moves time from one launch into the other and gave between +1.6 % and
// -3.6 % on the pair from one GPU to the next, both together -7 % on each (OPTLOG round 12 item 6) - and both when
//   * Z alone, 8 N ncomp bytes, exceeds the cache.  While all of Z fits, plain accesses keep part of it: at C5's shape with
//     N = 5e5 (Z 160 MB, the pair's three buffers 480 MB) the policy gained nothing (0.2137 against 0.2105 ms per step, and
//     0.2150 against 0.2152 on another GPU);
//   * the resident half, counted exactly from the tile geometry, fits the cache.  Measured at C5's shape: a half of 0.62 of the
//     cache (N = 1e6) -7.2 % per step, 0.93 of it (N = 1.3e6) -6.7 % with the inverse launch as fast as under the plain policy.
//     A half of 1.25 caches (N = 1.6e6) still gained 4.9 % / 6.0 % on the step, all of it in the forward launch, while the
//     inverse lost 7 % / 2 %: its loads miss, which is not what this policy is for - left to the plain policy until someone
//     measures beyond.
static inline int band_resident_policy(int64_t N, int64_t chunk_rows, int ncomp, int option) {
    if (option >= 0) return option & (BAND_POLICY_FORWARD | BAND_POLICY_INVERSE);
    const int64_t col = 8 * (int64_t)ncomp;          // bytes of a row across the components
    if (col * N <= TTM_LLC_BYTES) return 0;
    if (band_policy_resident_rows(N, chunk_rows) * col > TTM_LLC_BYTES) return 0;
    return BAND_POLICY_FORWARD | BAND_POLICY_INVERSE;
}
