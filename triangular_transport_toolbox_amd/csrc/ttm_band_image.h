// ttm_band_image.h - the resident-table IMAGE of a component's inverse table: the bytes k_band_inverse keeps in LDS per
// component (search parameters, the windowed table, the 16-bit bucket index), laid out once per coefficient vector by the
// kernel that builds the table (k_table_build_index, csrc/ttm_kernels.hip) so that the lookup kernel can copy them into LDS
// by DMA (k_band_inverse_ring, csrc/ttm_band.hip) instead of assembling them per workgroup and block: a block switch of
// k_band_inverse is a string of dependent round trips (header loads, two rounds of table loads, the per-bucket scan:
// 5.9 us of a 143 us launch at C5), the DMA of a group of images is issued a group of columns ahead and costs a barrier.
//
// image of one component, `tab_slot` doubles (a whole number of 16-byte units):
//   [wl, wh, bucket scale, bucket bias, int32 {entries per bucket at most, 0}, int32 {degenerate, 0} |
//    xs: the W table entries of the window [w0, w0 + W) + sentinels (+inf) up to Weven | bucket index: nb + 1 uint16, zero padded]
// exactly what the block prologue of k_band_inverse leaves in a table slot (the same values, the same bits).
//
// The SLOPE layout (BandImageSlot::slopes, chosen by band_ring_plan) puts Weven more doubles between xs and the bucket index:
//   [header | xs: Weven | slopes: Weven | bucket index]
// slopes[i] = band_interval_slope of the interval BELOW window entry i, (x, y) of table entries w0 + i - 1 and w0 + i - the
// first window entry takes the table entry in front of the window as its x_lo; 0 where there is no such interval (entry 0
// of the table, the sentinels).  The slope is a function of the table alone, so the lookup reads it instead of forming it per
// row (a reciprocal, its Newton step, two differences, a product and two LDS reads): the same operations in the same order,
// done once by the kernel that builds the table - the same bits.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "ttm_band_policy.h"

#define BAND_RT_HDR 6
#define BAND_RING_KMAX 24                             /* slots of the ring, at most */

// doubles of one image: header, the window's entries up to an even count, the bucket index (four uint16 per double, even).
// THE one copy of this geometry: the kernel that writes the images and every kernel that reads them take it from here.
struct BandImageSlot {
    int Weven, tab_slot;
    int slopes;                                       // 1: the slope layout
    size_t lds(int slots) const { return ((size_t)2 * Weven + (size_t)slots * tab_slot) * 8; }   // `slots` images next to the {E_i, y_i} pairs of the window
    int index_at() const { return BAND_RT_HDR + (slopes ? 2 : 1) * Weven; }                      // where the bucket index starts (doubles)
};
static inline BandImageSlot band_image_slot(int W, int nb, int slopes = 0) {
    const int Weven = (W + 4 + 1) & ~1;
    return {Weven, BAND_RT_HDR + (slopes ? 2 : 1) * Weven + (((nb + 1 + 3) / 4 + 1) & ~1), slopes ? 1 : 0};
}

struct BandRingPlan {
    int W, w0, Weven, tab_slot;                       // window [w0, w0 + W) of every table, doubles per image
    int R, G;                                         // ring of R slots, refilled G at a time (G = 0: every component resident, no refill)
    size_t lds;                                       // dynamic LDS of the launch
    int slopes;                                       // 1: the images carry the interval slopes (BandImageSlot)
};

// The plan of ONE layout (band_ring_plan below chooses between the two).  false: no ring kernel for this geometry and layout.
static inline bool band_ring_plan_layout(int T, int nb, int ncomp, size_t lds_per_cu, int window, int block, double wfrac, int slopes,
                                         BandRingPlan* pl) {
    if (T < 64 || T > 4096 || nb + 1 != 1024 || ncomp < 1) return false;
    auto fit = [&](int W) {                           // slots that fit next to the {E_i, y_i} pairs of the window
        const BandImageSlot s = band_image_slot(W, nb, slopes);
        if (s.lds(1) > lds_per_cu) return 0;
        int B = (int)((lds_per_cu - s.lds(0)) / ((size_t)s.tab_slot * 8));
        if (B > BAND_RING_KMAX) B = BAND_RING_KMAX;
        if (block > 0 && block < B) B = block;
        return B;
    };
    int W = T, w0 = 0;
    int B = fit(W);
    if (window > 0 || (window != 0 && B < ncomp)) {   // windowed tables when whole ones would need refills (or on request)
        int Ww = window > 0 ? (window < 16 ? 16 : window) : (int)(wfrac * T);
        if (Ww >= T) Ww = T - 1;
        Ww &= ~1;                                     // (even: the doubles per image then determine the window - what a lookup checks)
        const int Bw = fit(Ww);
        if (window > 0 || Bw > B) { W = Ww; w0 = (T - Ww) / 2; B = Bw; }
    }
    if (B <= 0) return false;
    pl->W = W; pl->w0 = w0;
    const BandImageSlot slot = band_image_slot(W, nb, slopes);
    pl->Weven = slot.Weven; pl->tab_slot = slot.tab_slot; pl->slopes = slot.slopes;
    if (pl->tab_slot % 2) return false;               // (16-byte units)
    if (ncomp <= B) { pl->R = ncomp; pl->G = 0; }
    else {
        const int G = 4;                              // (refills of 8 measured 2 % slower at C5: OPTLOG round 4, item 22)
        const int R = B / G * G;
        if (R < 3 * G) return false;                  // (a refill is certified one group after it is issued and used two groups on)
        pl->R = R; pl->G = G;
    }
    pl->lds = slot.lds(pl->R);
    return true;
}

// option band_slopes (ttm_options.h): -1 auto, 0 off, 1 on wherever the plan allows.  Auto: on (measured: OPTLOG round 16).
constexpr int BAND_SLOPES_AUTO = 1;

// The plan is a function of the table geometry, the number of components, the LDS of a CU and the options alone: the kernel
// that writes the images and the kernel that reads them compute it separately and agree.  false: no ring kernel for this geometry.
// The slope layout makes an image larger by Weven doubles (C5: 786 -> 1310, 14 slots beside the pairs instead of 24), so it is
// taken only where it leaves the KIND of plan alone:
//   * a refilled ring stays a legal refilled ring (R >= 3 G: 12 slots at C5, measured no slower than 24 - OPTLOG round 15), or
//   * every component is resident under both layouts (the window may differ: ten whole tables fit, ten whole tables with
//     their slopes do not, ten windowed ones do).
// It is NOT taken where it would turn a map that is fully resident today (G = 0, up to 24 components) into a refilled one, nor
// where today's layout has no plan: such geometries keep today's image and today's code.
static inline bool band_ring_plan(int T, int nb, int ncomp, size_t lds_per_cu, int window, int block, double wfrac, BandRingPlan* pl,
                                  int slopes_option = 0) {
    if (!band_ring_plan_layout(T, nb, ncomp, lds_per_cu, window, block, wfrac, 0, pl)) return false;
    if (slopes_option < 0) slopes_option = BAND_SLOPES_AUTO;
    BandRingPlan with;
    if (slopes_option > 0 && band_ring_plan_layout(T, nb, ncomp, lds_per_cu, window, block, wfrac, 1, &with) && (with.G == 0) == (pl->G == 0) &&
        (with.G == 0 || with.tab_slot <= 2048))            // (a refill copies an image as one 1 KB piece per wave of the lookup kernel: 16 waves)
        *pl = with;
    return true;
}

// The plan `pl` with `extra` bytes of LDS behind the {E_i, y_i} pairs (the column buffers of k_band_inverse_ring's ZD = 1)
// and at most `max_slots` slots (0: as many as fit): the SAME images - window and doubles per image are what the table
// kernel wrote - in a ring of fewer slots.  A ring without refill keeps every component whatever `max_slots`.  false: the
// slots left are fewer than the ring needs (every component when there is no refill, else the 3 G of band_ring_plan).
static inline bool band_ring_plan_with(const BandRingPlan& pl, size_t lds_per_cu, size_t extra, int max_slots, BandRingPlan* out) {
    const BandImageSlot slot = {pl.Weven, pl.tab_slot, pl.slopes};
    if (slot.lds(0) + extra > lds_per_cu) return false;
    const int B = (int)((lds_per_cu - extra - slot.lds(0)) / ((size_t)slot.tab_slot * 8));
    *out = pl;
    if (pl.G == 0) { if (B < pl.R) return false; }
    else {
        int R = (B < pl.R ? B : pl.R) / pl.G * pl.G;       // what fits
        if (R < 3 * pl.G) return false;
        if (max_slots > 0 && max_slots < R) R = (max_slots < 3 * pl.G ? 3 * pl.G : max_slots) / pl.G * pl.G;   // (a cap only lowers it, to 3 G at least)
        out->R = R;
    }
    out->lds = slot.lds(out->R) + extra;
    return true;
}

// Everything ttm_band::inverse decides about a k_band_inverse_ring launch once the images fit the plan `pl`: the cut, the
// cache policy, ZD and the ring it launches with.  THE one copy: the host entry point and the CPU program of the tests
// (tests/band_cut_gate.cpp) both call it.  ring_slots: option band_ring_slots (0 / -1: as many slots as fit).
struct BandRingLaunch {
    BandCut cut;
    bool pol, zd;                                     // POL = 1, ZD = 1
    BandRingPlan ring;                                // slots and dynamic LDS of the launch
};
static inline BandRingLaunch band_ring_launch(const BandRingPlan& pl, int64_t N, int cus, int ncomp, size_t lds_per_cu, int full_tiles,
                                              int resident, int zdma, int ring_slots) {
    BandRingLaunch l;
    l.cut = band_policy_cut(N, cus, full_tiles);
    l.pol = (band_resident_policy(N, l.cut.rows, ncomp, resident) & BAND_POLICY_INVERSE) != 0;
    const int slots = ring_slots > 0 ? ring_slots : 0;
    BandRingPlan with;
    // Z two columns ahead through LDS: the same images in the slots the two column buffers leave - never images with slopes
    // (they leave the buffers no room at C5, and k_band_inverse_ring has no such instantiation)
    l.zd = band_zdma_policy(N, l.cut, l.pol, !pl.slopes && band_ring_plan_with(pl, lds_per_cu, (size_t)BAND_ZDMA_LDS_BYTES, slots, &with), zdma);
    l.ring = pl;
    if (l.zd || (slots > 0 && band_ring_plan_with(pl, lds_per_cu, 0, slots, &with))) l.ring = with;
    return l;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void band_bucket_params(double lo, double hi, int nb, double& scale, double& bias) {
    scale = (double)nb / (hi - lo);                                           // (k_table_index: the same IEEE division)
    if (!(scale > 0.0 && scale < 1.0e300)) scale = 0.0;
    bias = -lo * scale;
}

// THE one definition of an interval's slope, interp1d's slope form (TM:4062-4065) with the difference floored (the tie at a
// flat start: include/ttm.h, THE TIE RULE): what the lookup kernels form per row and what band_image_write stores per interval.
__device__ __forceinline__ double band_interval_slope(double x_lo, double x_hi, double y_lo, double y_hi) {
    const double dx = fmax(x_hi - x_lo, 1e-300);
    double rc = __builtin_amdgcn_rcp(dx);
    rc = fma(fma(-dx, rc, 1.0), rc, rc);
    return (y_hi - y_lo) * rc;
}

// One workgroup writes the image of its component: xs (LDS, the T sorted table entries), bks (LDS, nb + 1 bucket starts as
// k_table_index computes them), red (LDS, one int, any value).  Every thread of the workgroup calls it.  ys (slope layout
// only - tab_slot tells): the T abscissae of the table, the values a lookup computes as i * step + y0 (y_last at T - 1) to
// the bit (include/ttm.h, THE ABSCISSAE: a lookup that passes h_y_affine vouches for exactly that).
__device__ inline void band_image_write(const double* xs, const int* bks, int* red, int T, int nb, double lo, double hi, int w0, int W,
                                        int Weven, int tab_slot, double* __restrict__ img, const double* __restrict__ ys = nullptr) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nbd = ((nb + 1 + 3) / 4 + 1) & ~1;       // doubles of the bucket index (band_image_slot)
    const bool slopes = tab_slot == BAND_RT_HDR + 2 * Weven + nbd;
    const int index_at = tab_slot - nbd;
    if (tid == 0) *red = 0;
    __syncthreads();
    // entries per bucket, at most, over the buckets that reach into the window
    int per = 0;
    for (int b = tid; b < nb; b += nt) {
        const int b0 = bks[b] & 0xffff, b1 = bks[b + 1] & 0xffff;
        if (b1 > w0 && b0 < w0 + W) per = b1 - b0 > per ? b1 - b0 : per;
    }
    if (per > 0) atomicMax(red, per);
    __syncthreads();
    per = *red;
    const int pm = per > 1 ? per : 1;
    const bool deg = pm + 3 >= W || per > 4;          // (more entries in a bucket than the resident search compares: every row by the outlier path)
    auto xw = [&](int i) { return i < W ? xs[w0 + i] : (double)INFINITY; };
    if (tid == 0) {
        double scale, bias;
        band_bucket_params(lo, hi, nb, scale, bias);
        img[0] = deg ? xw(1) : xw(pm);
        img[1] = deg ? xw(1) : xw(W - 2);
        img[2] = scale; img[3] = bias;
        int* ih = (int*)(img + 4);
        ih[0] = per; ih[1] = 0; ih[2] = deg ? 1 : 0; ih[3] = 0;
    }
    for (int i = tid; i < Weven; i += nt) img[BAND_RT_HDR + i] = xw(i);
    if (slopes)
        for (int i = tid; i < Weven; i += nt) {
            const int g = w0 + i;                     // the interval below table entry g
            img[BAND_RT_HDR + Weven + i] = i < W && g >= 1 ? band_interval_slope(xs[g - 1], xs[g], ys[g - 1], ys[g]) : 0.0;
        }
    // bucket index: four uint16 per double, zero behind entry nb
    for (int i = tid; i < nbd; i += nt) {
        unsigned long long pk = 0;
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * i + j;
            const unsigned long long v = q <= nb ? (deg ? (unsigned)(w0 + 1) : (unsigned)bks[q]) & 0xffffu : 0u;
            pk |= v << (16 * j);
        }
        img[index_at + i] = __longlong_as_double((long long)pk);
    }
}
#endif
