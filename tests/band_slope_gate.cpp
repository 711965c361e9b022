// Prints which image layout the planner of k_band_inverse_ring (csrc/ttm_band_image.h: band_ring_plan) chooses for the sizes
// on the command line - today's, or the one with the interval slopes - and the launch that follows from it.  A CPU program:
// the headers are plain C++.  tests/test_band_slopes.py compiles and runs it.
//     band_slope_gate T nb ncomp lds_per_cu N cus band_slopes band_zdma
//         -> "<ring?> <slopes> <R> <G> <W> <w0> <doubles per image> <HDR + (1 or 2) Weven + index doubles> <lds>
//             | <ZD> <R> <slopes> <lds> of the launch"
#include <stdio.h>
#include <stdlib.h>

#include "ttm_band_image.h"
#include "ttm_band_policy.h"

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const int T = atoi(argv[1]), nb = atoi(argv[2]), ncomp = atoi(argv[3]);
    const size_t lds = (size_t)atoll(argv[4]);
    const int64_t N = atoll(argv[5]);
    const int cus = atoi(argv[6]), slopes = atoi(argv[7]), zdma = atoi(argv[8]);
    BandRingPlan pl = {};
    const bool ring = band_ring_plan(T, nb, ncomp, lds, -1, -1, 0.52, &pl, slopes);
    if (!ring) {
        printf("0 0 0 0 0 0 0 0 0 | 0 0 0 0\n");
        return 0;
    }
    // the doubles of an image counted by hand: header, xs (and the slopes), four 16-bit bucket starts per double, even
    const int index = ((nb + 1 + 3) / 4 + 1) & ~1;
    const int counted = BAND_RT_HDR + (pl.slopes ? 2 : 1) * pl.Weven + index;
    // the launch: the function ttm_band::inverse calls (resident policy and whole tiles forced, so that only the ring decides ZD)
    const BandRingLaunch rl = band_ring_launch(pl, N, cus, ncomp, lds, 1, 3, zdma, 0);
    printf("1 %d %d %d %d %d %d %d %zu | %d %d %d %zu\n", pl.slopes, pl.R, pl.G, pl.W, pl.w0, pl.tab_slot, counted, pl.lds, rl.zd ? 1 : 0, rl.ring.R,
           rl.ring.slopes, rl.ring.lds);
    return 0;
}
