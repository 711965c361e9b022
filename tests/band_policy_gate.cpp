// Prints the decision of band_resident_policy (csrc/ttm_band_policy.h) for the sizes on the command line - a CPU program: the
// header is plain C++.  tests/test_band_resident.py compiles and runs it.
//     band_policy_gate N ncomp option [chunk_rows]
// chunk_rows omitted: what ttm_band.hip's chunk_grid plans for the 256 CUs of an MI355X (N / 256 rounded up to 32 rows).
// Output: "<decision> <resident rows> <chunk rows>"
#include <stdio.h>
#include <stdlib.h>

#include "ttm_band_policy.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int64_t N = atoll(argv[1]);
    const int ncomp = atoi(argv[2]), option = atoi(argv[3]);
    int64_t rows = argc > 4 ? atoll(argv[4]) : 0;
    if (rows <= 0) rows = ((N + 255) / 256 + 31) / 32 * 32;
    printf("%d %lld %lld\n", band_resident_policy(N, rows, ncomp, option), (long long)band_policy_resident_rows(N, rows), (long long)rows);
    return 0;
}
