// ttm_band.h - internal interface of csrc/ttm_band.hip (the kernels of banded U-form maps) to csrc/ttm_kernels.hip.
//
// A BANDED map (BASELINE config 5, Markov-type maps): the columns of the components are consecutive and every
// nonmonotone group of component k reads a column kc-1 .. kc-LAG (LAG <= TTM_P_LAG_MAX), the monotone part of every
// component is a special-term spline, one linear term of its own variable, or both (no other polynomial / Hermite-function
// terms of the own variable).  Such a map is evaluated in PUSH form: walking the
// columns in order, the value x_c of a column is used at once for everything that depends on it -
//
//     S at column c          = pend[0] + own1_c x_c + G_c(x_c)         (G_c: the component's spline, own1_c: slope of its linear term)
//     pend[l], l = 0..LAG-2  = pend[l+1] + f_{c+l+1, c}(x_c)           (contribution to the component l+1 columns on)
//     pend[LAG-1]            = c0_{c+LAG} + f_{c+LAG, c}(x_c)
//
// so a row carries LAG running sums instead of LAG cached columns with their exp(-x^2/4), and one step is straight-line
// code.  The push records ("P section" of the U section, include/ttm.h) hold, per column, the coefficients of the
// groups that READ the column; ttm_fold builds them behind the hot records.
#pragma once

#include <stdint.h>

#include "../../include/ttm.h"

namespace ttm_band {

// build the P section from the H section (device, on `stream`); also writes the local-coordinate offset of every spline
// column into its padding slot.  U: the U section of the folded-coefficient buffer.
int build_records(const ttm_program* p, double* U, void* stream);

// doubles per push record of degree class `cls` with `lag` groups (what u_p_stride must be)
int record_stride(int cls, int lag);

// can [k0, k1) of this program run through the band kernels?
bool usable(const ttm_program* p, int k0, int k1);

// forward map of the components [k0, k1): Z and / or the fused log-determinant and sum of squares (`block` > 0: at most that
// many components' splines resident at a time; `resident`: option band_resident - the cache policy of k_band_forward's column
// streams, csrc/ttm_band_policy.h; `full_tiles`: option band_full_tiles - the cut of a k_band_forward launch, as inverse()'s)
int forward(const ttm_program* p, const double* U, int k0, int k1, const double* Xsoa, int64_t ldx, int64_t N, double* Zsoa,
            int64_t ldz, double* logdet, const double* sigma, double* sumsq, int cus, size_t lds_per_cu, int block, int resident, int full_tiles,
            void* stream, const char** kernel_name);

// table inverse (resident windowed tables, as k_inverse_rt) in push form
// img: the resident-table images of the components (image_plan; written by k_table_build_index) or nullptr
// resident: option band_resident - the cache policy of k_band_inverse_ring's column streams (csrc/ttm_band_policy.h)
// full_tiles, zdma, ring_slots: options band_full_tiles, band_zdma, band_ring_slots - the cut of a k_band_inverse_ring launch, its
// ZD and the slots of its ring (same header); slopes: option band_slopes - images with interval slopes where the plan allows
// (csrc/ttm_band_image.h: band_ring_plan), the value the images were built under
int inverse(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx,
            int64_t N, const double* tab_x, int T, const double* y_affine, const double* tmin, const double* tmax, const int32_t* bkt,
            int nb, const double* img, int img_doubles, int cus, size_t lds_per_cu, int window, int block, int resident, int full_tiles, int zdma,
            int ring_slots, int slopes, void* stream, const char** kernel_name);

// safeguarded Newton root search (sample_newton, csrc/ttm_eval.h: bracket +-2, window doubling, |S - z| <= 1e-9, at most 100
// trial points) in push form: the monotone part is the component's resident spline (+ its linear own term), no
// tables.  Conditioning columns (if any) are read from Xsoa.  iters: as ttm_inverse_newton.  1: declined
int newton(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
           int32_t* iters, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name);

// the reference's bisection (sample_bisect, csrc/ttm_eval.h: bracket +-2, window shifts, midpoints until |S - z| <= 1e-9 or 100
// of them, the last midpoint returned; no cap - the capped replay of sample 0 stays with the generic kernel) in push form, planned
// as newton().  iters: as ttm_inverse_bisect (midpoints).  1: declined
int bisect(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
           int32_t* iters, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name);

// would bisect() take these arguments?  Its checks without a launch (the entry point asks before it splits a call)
bool bisect_plans(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
                  int32_t* iters, int cus, size_t lds_per_cu, int block);

// score of the pullback density of the whole map (csrc/ttm_score.h, include/ttm.h: ttm_score) in push form: one sweep over the
// columns, G column j complete and stored at step j + lag.  g_scale / ld_affine: nullable, as ttm_score.  Planned as the long
// kernels (a chunk of rows per workgroup, blocks of resident splines) for every map usable() accepts.  1: declined
int score(const ttm_program* p, const double* U, const double* Xsoa, int64_t ldx, int64_t N, double* Gsoa, int64_t ldg, const double* g_scale,
          const double* ld_affine, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name);

// forward map (+ log-determinant / sum of squares) and the table inverse of the image, in ONE launch, for maps of a few components
// (k_band_few_roundtrip): Z (nullable) = S(X), Xr = S^-1(S(X)) - conditioning columns are read from X.  Without `force` only the
// shapes the one launch is faster for (reach <= 2 columns, no density terms); 1: declined
int roundtrip(const ttm_program* p, const double* U, int k0, int k1, const double* Xsoa, int64_t ldx, int64_t N, double* Zsoa, int64_t ldz,
              double* Xr, int64_t ldr, double* logdet, const double* sigma, double* sumsq, const double* tab_x, int T, const double* y_affine,
              const double* tmin, const double* tmax, const int32_t* bkt, int nb, int cus, size_t lds_per_cu, bool force, void* stream,
              const char** kernel_name);

// does the table inverse of [k0, k1) take resident-table images (csrc/ttm_band_image.h) for this table geometry?  The window
// [w0, w0 + W) of every table and the doubles per image (the table-building kernel writes them, `inverse` reads them; with the
// interval slopes where option band_slopes and the plan allow: the doubles per image tell the layout)
bool image_plan(const ttm_program* p, int k0, int k1, int T, int nb, size_t lds_per_cu, int window, int block, int slopes, int* w0, int* W,
                int* tab_slot);

// TEST HOOK (ttm_math_probe, include/ttm.h): out[i] = f(a[i] [, b[i]]) for the primitives private to csrc/ttm_band.hip -
// `which` one of TTM_PROBE_BAND_* (the caller has checked it and the pointers; n >= 1).  The pair table is staged by the
// forward kernels' loader, the Taylor coefficients are g_band_taylor.
int math_probe(int which, const double* a, const double* b, int64_t n, double* out, void* stream, const char** kernel_name);

}  // namespace ttm_band
