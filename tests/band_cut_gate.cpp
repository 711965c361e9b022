// Prints what the planner of k_band_forward / k_band_inverse_ring (csrc/ttm_band_policy.h, csrc/ttm_band_image.h) decides for
// the sizes on the command line - a CPU program: both headers are plain C++.  tests/test_band_zdma.py compiles and runs it.
//     band_cut_gate cut N cus band_full_tiles
//         -> "<chunk rows> <workgroups> <full-tile rule: 0 / 1> <resident rows of that cut>"
//     band_cut_gate ring T nb ncomp lds_per_cu N cus band_full_tiles band_resident band_zdma band_ring_slots
//         -> "<ring?> <R> <G> <lds> | <ring beside the column buffers?> <R> <G> <lds> | <ZD> | <R> <lds> of the launch"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ttm_band_image.h"
#include "ttm_band_policy.h"

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "cut")) {
        const int64_t N = atoll(argv[2]);
        const BandCut c = band_policy_cut(N, atoi(argv[3]), atoi(argv[4]));
        printf("%lld %lld %d %lld\n", (long long)c.rows, (long long)c.grid, c.full_tiles ? 1 : 0, (long long)band_policy_resident_rows(N, c.rows));
        return 0;
    }
    if (argc == 12 && !strcmp(argv[1], "ring")) {
        const int T = atoi(argv[2]), nb = atoi(argv[3]), ncomp = atoi(argv[4]);
        const size_t lds = (size_t)atoll(argv[5]);
        const int64_t N = atoll(argv[6]);
        const int cus = atoi(argv[7]), full_tiles = atoi(argv[8]), resident = atoi(argv[9]), zdma = atoi(argv[10]), slots = atoi(argv[11]);
        BandRingPlan pl = {}, zpl = {};
        const bool ring = band_ring_plan(T, nb, ncomp, lds, -1, -1, 0.52, &pl);
        const bool zring = ring && band_ring_plan_with(pl, lds, (size_t)BAND_ZDMA_LDS_BYTES, slots > 0 ? slots : 0, &zpl);
        // the launch: the function ttm_band::inverse calls
        BandRingLaunch rl = {};
        if (ring) rl = band_ring_launch(pl, N, cus, ncomp, lds, full_tiles, resident, zdma, slots);
        const bool zd = rl.zd;
        const BandRingPlan launch = rl.ring;
        printf("%d %d %d %zu | %d %d %d %zu | %d | %d %zu\n", ring ? 1 : 0, pl.R, pl.G, pl.lds, zring ? 1 : 0, zring ? zpl.R : 0, zring ? zpl.G : 0,
               zring ? zpl.lds : (size_t)0, zd ? 1 : 0, ring ? launch.R : 0, ring ? launch.lds : (size_t)0);
        return 0;
    }
    return 2;
}
