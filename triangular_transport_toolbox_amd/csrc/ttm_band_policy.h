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
