// ttm_band.hip - forward map and table inverse of BANDED U-form maps in push form (ttm_band.h, include/ttm.h
// "push records").  BASELINE config 5 (d = 40, band 2, order 3, N = 1e6) is the map these kernels are written for;
// reference: transport_map.py:2391-2567 (map, s), 3987-4084 (table root search).
//
// What differs from k_forward_hl / k_inverse_rt (csrc/ttm_kernels.hip), and why (profiles/r03_*):
//   * both were VALU-issue bound at ~50 % utilisation with every VALU instruction costing the same ~4 cycles whatever
//     its type (tools/micro/valu_costs.hip): the lever is the instruction COUNT per component evaluation and the
//     number of basic blocks / dependent LDS round trips a step is cut into;
//   * push form: a row carries LAG running sums (registers) instead of LAG columns with their exp(-x^2/4): no column
//     cache in LDS, no loader waves, no barrier per step, one straight-line step per column;
//   * exp(-x^2/4) = E_i exp(w) from the nearest point of a fixed grid (801 pairs {E_i, y_i/4}, correctly rounded,
//     csrc/ttm_band_etab.h) and the degree-7 Taylor polynomial of exp(w), |w| <= 0.025 for |x| <= 5: 15 instructions
//     instead of 22, relative error <= 2.2e-16 + 4e-18 (|x| <= 5), no clamp / ldexp / NaN repair;
//   * the spline's column and local coordinate come from one fma + cvt + med3 + mad and one fma against a per-column
//     offset read with the coefficients (slot 12 of the column): 5 instructions instead of 9.
// One workgroup of 1024 threads per CU owns a contiguous chunk of rows; a thread carries four rows (two adjacent pairs:
// 16-byte accesses) through all columns; the splines of all components (140 KB at C5) are resident in LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

#include "ttm_band.h"
#include "ttm_band_etab.h"
#include "ttm_band_image.h"
#include "ttm_band_policy.h"

namespace ttm_band {

typedef const __attribute__((address_space(4))) double* cdbl_p;      // uniform data: scalar loads
typedef const __attribute__((address_space(4))) int* cint_p;
struct __attribute__((aligned(16))) D2 { double x, y; };

__device__ const double g_band_etab[2 * TTM_BAND_ET_N] = { TTM_BAND_ETAB_VALUES };
// Taylor coefficients of exp(w): 1/7! .. 1/2! (scalar operands of the fma chain)
__device__ double g_band_taylor[6] = {1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5};

__host__ __device__ constexpr int cls_db(int cls) { return cls == 1 ? 3 : (cls == 2 ? 5 : (cls == 3 ? 7 : 10)); }   // (class 4: few-component kernels only)
__host__ __device__ constexpr int cls_da(int cls) { return cls == 1 ? 1 : (cls == 2 ? 5 : (cls == 3 ? 7 : 10)); }
__host__ __device__ constexpr int cls_gs(int cls) { return cls == 1 ? 8 : (cls == 2 ? 16 : 24); }
__host__ __device__ constexpr int cls_gp(int cls) { return cls_db(cls) + 1 + cls_da(cls); }
__host__ __device__ constexpr int rec_stride(int cls, int lag) { return (TTM_P_HDR + lag * cls_gp(cls) + 7) / 8 * 8; }

#define BAND_ET_DOUBLES (2 * TTM_BAND_ET_N)          /* 12 816 bytes: a multiple of 16 */
#define BAND_CT 1024                                 /* threads per workgroup */
#define BAND_NS 4                                    /* rows per thread: pairs (2t, 2t+1) of the two halves of a tile */
#define BAND_PF 1                                    /* columns requested ahead of the one being evaluated */
static_assert(BAND_POLICY_TILE_ROWS == BAND_NS * BAND_CT && BAND_POLICY_HALF_ROWS == 2 * BAND_CT && BAND_NS == 4,
              "ttm_band_policy.h counts the rows of pair slot 0 of these tiles");

// One LDS-DMA instruction (16 bytes per lane: the wave's 1 KB lands at lds_wave_base, an LDS byte address, lane after lane),
// written in assembly so that the COMPILER DOES NOT KNOW IT: with a global_load_lds it knows to be in flight hipcc waits for
// vmcnt(0) at the next use of any ordinary load (the column prefetch would be drained every step).  Unknown to it, its
// counted waits are merely one stricter per copy among the younger operations: place the copy behind the step's wait for z,
// and that wait retires the PREVIOUS step's copy (a whole step old) and nothing else.
__device__ __forceinline__ void band_dma16(const void* g, unsigned int lds_wave_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_wave_base) : "m0");
}
// ... with the non-temporal bit (the column stream of Z that is not to stay on-die: band_z_nt)
__device__ __forceinline__ void band_dma16_nt(const void* g, unsigned int lds_wave_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(g), "s"(lds_wave_base) : "m0");
}
__device__ __forceinline__ unsigned int band_lds_addr(const void* p) {
    return (unsigned int)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// n doubles (even; both sides 16-byte aligned) from memory into LDS: every 16-byte unit requested at once by DMA, then waited
// for - one memory round trip.  (A loop of load / store pairs through registers is compiled to load, wait, store per trip:
// nine dependent round trips for the 140 KB of splines of C5.)  The caller's barrier publishes the bytes.
template <bool WAIT = true>
__device__ __forceinline__ void band_stage(double* lds_dst, const double* src, int n) {
    const int units = n >> 1;
    const unsigned int base = band_lds_addr(lds_dst);
    for (int u0 = 0; u0 < units; u0 += BAND_CT) {
        const int u = u0 + (int)threadIdx.x;
        if (u < units) band_dma16(src + 2 * (size_t)u, __builtin_amdgcn_readfirstlane(base + (unsigned int)(u0 + ((int)threadIdx.x & ~63)) * 16u));
    }
    if (WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---------------------------------------------------------------------------
// push records from the hot records (one workgroup of 64 threads per record)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_band_records(const int* __restrict__ ucomp, const int* __restrict__ ugrp, double* __restrict__ U,
                                                     int64_t h_off, int cls, int ng, int64_t p_off, int lag, int ps, int D) {
    const int r = blockIdx.x, k = r - lag, t = threadIdx.x;
    const int DB = cls_db(cls), DA = cls_da(cls), GS = cls_gs(cls), GP = cls_gp(cls);
    const int hs = TTM_H_HDR + ng * GS;
    double* rec = U + p_off + (int64_t)r * ps;
    auto hot = [&](int kk) { return U + h_off + (int64_t)kk * hs; };
    // the linear term of a component's own variable, if it has one (maps of a few components: A[0], A[1] of the group behind
    // the nonmonotone ones in the component's U-form block)
    auto own = [&](int kk, int deg) {
        const int* uc = ucomp + kk * TTM_UC_LEN;
        return (uc[TTM_UC_FLAGS] & TTM_UCF_OWN) ? U[uc[TTM_UC_DBL_OFF] + 4 + TTM_U_GSTRIDE * uc[TTM_UC_N_GRP] + TTM_U_GHALF + deg] : 0.0;
    };
    // the group of component kk that reads the column `lg` columns in front of it: index into its hot record, -1: none
    auto group_at = [&](int kk, int lg) {
        const int* uc = ucomp + kk * TTM_UC_LEN;
        for (int g = 0; g < uc[TTM_UC_N_GRP]; ++g)
            if (uc[TTM_UC_KC] - ugrp[(uc[TTM_UC_GRP_OFF] + g) * TTM_UG_LEN + TTM_UG_VAR] == lg) return g;
        return -1;
    };
    for (int i = t; i < ps; i += 64) {
        double v = 0.0;
        if (i < 2) {                                          // chain start of the component `lag` columns on
            const int kk = k + lag;
            if (kk >= 0 && kk < D) {
                const double* h = hot(kk);
                v = i == 0 ? h[2] : h[7];
                const int* uc = ucomp + kk * TTM_UC_LEN;
                for (int g = 0; g < uc[TTM_UC_N_GRP]; ++g) v += h[TTM_H_HDR + g * GS + 2 + DB];      // A[0] of the group
                if (i == 0) v += own(kk, 0);                  // (the monotone part's own constant: forward map only)
            }
        } else if (i < TTM_P_HDR) {
            if (k >= 0) {
                const double* h = hot(k);
                const int* uc = ucomp + k * TTM_UC_LEN;
                if (i == 2) v = h[3] + 1.0;
                else if (i == 3) v = h[4];
                else if (i == 4) v = h[5];
                else if (i == 5) { int2 w = {uc[TTM_UC_NI], uc[TTM_UC_TAB_OFF]}; v = *(double*)&w; }
                else if (i == 6) { int2 w = {k, 0}; v = *(double*)&w; }
                else if (i == 7) v = own(k, 1);
            } else if (i == 6) { int2 w = {-1, 0}; v = *(double*)&w; }
        } else {
            const int l = (i - TTM_P_HDR) / GP, j = (i - TTM_P_HDR) % GP;
            const int kk = k + l + 1;
            if (l < lag && kk >= 0 && kk < D) {
                const int g = group_at(kk, l + 1);
                if (g >= 0) {
                    const double* gr = hot(kk) + TTM_H_HDR + g * GS;
                    v = j <= DB ? gr[1 + j] : gr[2 + DB + (j - DB)];              // B[j] | A[j - DB], j - DB = 1..DA
                }
            }
        }
        rec[i] = v;
    }
    if (k >= 0) {                                             // local-coordinate offsets of the spline columns
        const double* h = hot(k);
        const int* uc = ucomp + k * TTM_UC_LEN;
        double* tab = U + uc[TTM_UC_TAB_OFF];
        for (int c = t; c < uc[TTM_UC_NI]; c += 64) tab[c * TTM_U_TSTRIDE + 12] = fma(2.0, h[3], -(double)(2 * c - 1));
    }
}

// column stream accesses: 16 bytes per lane, plain or non-temporal (NT: `nt` on the instruction - the line does not allocate
// in the Infinity Cache).  Which of them a long kernel's streams take is its policy POL (k_band_forward, k_band_inverse_ring;
// ttm_band_policy.h): POL = 0 loads and stores plainly - what one launch leaves in the Infinity Cache is what the next one
// reads, as long as the pair's buffers fit it; POL = 1 lets only pair slot 0 of every tile allocate (band_z_nt) and
// streams everything else past it.  The few-component kernels' column stores are non-temporal; every other kernel is plain.
template <bool NT>
__device__ __forceinline__ void band_store2(char* p, double a, double b) {
    typedef double v2 __attribute__((ext_vector_type(2)));
    const v2 v = {a, b};
    if (NT) __builtin_nontemporal_store(v, (v2*)p);
    else *(v2*)p = v;
}
template <bool NT = false>
__device__ __forceinline__ D2 band_load2(const char* p) {
    typedef double v2 __attribute__((ext_vector_type(2)));
    v2 v;
    if (NT) v = __builtin_nontemporal_load((const v2*)p);
    else v = *(const v2*)p;
    const D2 r = {v.x, v.y};
    return r;
}
// POL = 1: the rows of pair slot q = 0 - the first half of every tile - are the part of Z that stays in the Infinity Cache from
// the forward map to the inverse; is the access of Z in slot Q non-temporal?
template <int POL, int Q> constexpr bool band_z_nt = POL != 0 && Q != 0;
// f(std::integral_constant<int, q>) for q = 0 .. N - 1: the loop over a thread's pair slots where the slot has to be a CONSTANT OF
// THE TYPE SYSTEM.  The policy of an access is part of the instruction; chosen by `if (q ...)` on the counter of an unrolled loop, the
// two accesses of one address are merged into one plain access before the loop is unrolled (seen in the assembly: no `nt` left).
template <class F, int... Q>
__device__ __forceinline__ void band_slots_seq(F& f, std::integer_sequence<int, Q...>) { (f(std::integral_constant<int, Q>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void band_slots(F&& f) { band_slots_seq(f, std::make_integer_sequence<int, N>{}); }

// ---------------------------------------------------------------------------
// per-row pieces of a step
// ---------------------------------------------------------------------------
__device__ __forceinline__ int band_med3(int v, int lo, int hi) {             // clamp(v, lo, hi), lo <= hi
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(lo), "s"(hi));
    return r;
}
__device__ __forceinline__ double band_absmin(double x, double hi) {            // min(|x|, hi); NaN -> hi
    double r;
    asm("v_min_f64 %0, |%1|, %2" : "=v"(r) : "v"(x), "s"(hi));
    return r;
}

// exp(-x^2/4) from the resident pair table
__device__ __forceinline__ double band_expq(const double* etab, double x, cdbl_p kt) {
    const double xe = band_absmin(x, TTM_BAND_ET_XMAX);
    const unsigned int i = (unsigned int)(int)fma(xe, TTM_BAND_ET_INV_STEP, 0.5);
    const D2 ey = *(const D2*)((const char*)etab + (i << 4));
    const double dq = fma(xe, -0.25, ey.y);                   // -(|x| - y_i) / 4
    const double sm = fma(ey.y, 4.0, xe);                     // y_i + |x|
    const double w = dq * sm;
    double p = fma(kt[0], w, kt[1]);
    p = fma(p, w, kt[2]);
    p = fma(p, w, kt[3]);
    p = fma(p, w, kt[4]);
    p = fma(p, w, kt[5]);
    p = fma(p, w, 1.0);
    p = fma(p, w, 1.0);
    return ey.x * p;
}

// pushes of one column value: pend[l] <- pend[l+1] (or the chain start) + group l of the record; g: the LAG group
// blocks of the record (uniform), E = exp(-x^2/4)
template <int DB, int DA, int LAG, class G>
__device__ __forceinline__ void band_push(const G& g, double start, double x, double E, double (&pend)[LAG]) {
    constexpr int GP = DB + 1 + DA;
#pragma unroll
    for (int l = 0; l < LAG; ++l) {
        const auto c = &g[l * GP];
        double b = c[DB];
#pragma unroll
        for (int i = DB - 1; i >= 0; --i) b = fma(b, x, c[i]);
        double a = c[DB + DA];
#pragma unroll
        for (int i = DA - 1; i >= 1; --i) a = fma(a, x, c[DB + i]);
        a = fma(a, x, l + 1 < LAG ? pend[l + 1] : start);
        pend[l] = fma(E, b, a);
    }
}

// the same for the kernels of maps with a few components: only the first LAGE groups of a record (no group of the sweep
// reaches further back), and without the plain polynomials when no group has any (PLAIN false).  GP: doubles per group
// of the record.
template <int DB, int DA, int GP, int LAGE, bool PLAIN, class G>
__device__ __forceinline__ void band_push_e(const G& g, double start, double x, double E, double (&pend)[LAGE]) {
#pragma unroll
    for (int l = 0; l < LAGE; ++l) {
        const auto c = &g[l * GP];
        double b = c[DB];
#pragma unroll
        for (int i = DB - 1; i >= 0; --i) b = fma(b, x, c[i]);
        double a = l + 1 < LAGE ? pend[l + 1] : start;
        if (PLAIN) {
            double q = c[DB + DA];
#pragma unroll
            for (int i = DA - 1; i >= 1; --i) q = fma(q, x, c[DB + i]);
            a = fma(q, x, a);
        }
        pend[l] = fma(E, b, a);
    }
}

// the special-term spline of a component at x: tab = the component's resident table, spl = {1 - t_lo/h, 1/h, 2/h}
__device__ __forceinline__ double band_spline(const double* tab, int nI, double sp_a, double sp_b, double sp_ds, double x) {
    const int col = band_med3((int)fma(x, sp_b, sp_a), 0, nI - 1);
    const double* cp = (const double*)((const char*)tab + __umul24((unsigned int)col, TTM_U_TSTRIDE * 8));
    double c[12];
#pragma unroll
    for (int i = 0; i < 12; i += 2) { const D2 v = *(const D2*)(cp + i); c[i] = v.x; c[i + 1] = v.y; }
    const double s = fma(x, sp_ds, cp[12]);
    double m = c[11];
#pragma unroll
    for (int i = 10; i >= 0; --i) m = fma(m, s, c[i]);
    return m;
}

// ---------------------------------------------------------------------------
// forward map
// ---------------------------------------------------------------------------
// the two rows of pair slot q of a step: S, the pushes, the store (NT: non-temporal).  rec: the step's record; xc: its column.
// What band_forward_tile's POL = 1 steps call; its POL = 0 steps have the same statements written out (see there)
template <int CLS, int LAG, bool FULL, bool OWN, bool NT>
__device__ __forceinline__ void band_forward_rows(int q, const D2 (&xc)[BAND_NS / 2], double (&pend)[BAND_NS][LAG], cdbl_p rec, double start, double sp_a,
                                                  double sp_b, double sp_ds, double own1, int nI, const double* tab, const double* etab, cdbl_p kt,
                                                  unsigned int tbase, char* zcol, unsigned int c1_32) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), HALF = 2 * BAND_CT;
    double zv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int e = 2 * q + h;
        const double x = h ? xc[q].y : xc[q].x;
        const double m = (!OWN || nI > 0) ? band_spline(tab, nI, sp_a, sp_b, sp_ds, x) : 0.0;
        const double E = band_expq(etab, x, kt);
        zv[h] = OWN ? fma(own1, x, pend[e][0] + m) : pend[e][0] + m;     // (x 0 too: a NaN / infinite sample stays NaN)
        band_push<DB, DA, LAG>(rec + TTM_P_HDR, start, x, E, pend[e]);
    }
    const unsigned int n = tbase + (unsigned int)(q * HALF);
    const D2 o = {zv[0], zv[1]};
    char* zp = zcol + (size_t)(n * 8u);
    if (FULL || n + 1 < c1_32) band_store2<NT>(zp, o.x, o.y);
    else if (n < c1_32) *(double*)zp = o.x;
    __builtin_amdgcn_sched_barrier(0);
}

// the columns [kb, ke) of one tile; FULL: every row of the tile exists (unmasked stores); OWN: some component of the map has
// a linear term of its own variable next to its spline or instead of it (slot [7] of the record; NI = 0: no spline);
// POL = 1: X is loaded non-temporally, Z stored plainly in pair slot 0 and non-temporally in slot 1 (band_z_nt)
template <int CLS, int LAG, bool FULL, bool OWN, int POL = 0>
__device__ __forceinline__ void band_forward_tile(cdbl_p P, cdbl_p kt, const double* etab, const double* tabs, int tab0, int kb, int ke,
                                                  const char* xcol, int64_t ldxb, char* zcol, int64_t ldzb, unsigned int tbase,
                                                  const unsigned int (&roff)[BAND_NS / 2], unsigned int c1_32,
                                                  double (&pend)[BAND_NS][LAG]) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, HALF = 2 * BAND_CT;
    // The column stream is latency bound (a step is shorter than a loaded memory round trip: profiles/r03_*): the column
    // of step j + PF is requested at the top of step j, PF + 1 register sets take turns (steps are issued PF + 1 at a time
    // with the roles rotated, so no set is ever copied).
    constexpr int PF = BAND_PF, RING = PF + 1;
    D2 xr[RING][NP];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const char* xc0 = xcol + (int64_t)(kb + i < ke ? i : 0) * ldxb;
#pragma unroll
        for (int q = 0; q < NP; ++q) xr[i][q] = band_load2<POL != 0>(xc0 + roff[q]);
    }
    cdbl_p rec = P + (int64_t)(kb + LAG) * PS;
    auto step = [&](int j, const D2 (&xc)[NP], D2 (&xn)[NP]) {
        {
            const char* xnext = j + PF < ke ? xcol + PF * ldxb : xcol;        // (past the block: a harmless re-read)
#pragma unroll
            for (int q = 0; q < NP; ++q) xn[q] = band_load2<POL != 0>(xnext + roff[q]);
        }
        __builtin_amdgcn_sched_barrier(0);                    // (the scheduler would sink the loads to the end of the step)
        // ---- uniform data of the step ------------------------------------------------------------------------
        const double start = rec[0], sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4];
        const double own1 = OWN ? rec[7] : 0.0;
        cint_p ri = (cint_p)rec;
        const int nI = ri[10];
        const double* tab = tabs + (ri[11] - tab0);
        // ---- row by row (two of them scheduled together: each needs 24 registers for its coefficients; the waves of the
        // SIMD, not the rows of a thread, fill each other's latencies) -------------------------------------------------
        if constexpr (POL == 0) {
            // (band_forward_rows<..., false>, written out: called as a function - or a lambda - in this loop, the same statements
            // moved the spills of k_band_forward<2, 2, true> and <3, 2, true>, 29 -> 33 and 28 -> 29 VGPRs, scratch 116 -> 180 bytes:
            // OPTLOG round 12 item 3.  The plain policy keeps the code it was measured with; a change to a row goes into both)
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                double zv[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int e = 2 * q + h;
                    const double x = h ? xc[q].y : xc[q].x;
                    const double m = (!OWN || nI > 0) ? band_spline(tab, nI, sp_a, sp_b, sp_ds, x) : 0.0;
                    const double E = band_expq(etab, x, kt);
                    zv[h] = OWN ? fma(own1, x, pend[e][0] + m) : pend[e][0] + m;     // (x 0 too: a NaN / infinite sample stays NaN)
                    band_push<DB, DA, LAG>(rec + TTM_P_HDR, start, x, E, pend[e]);
                }
                const unsigned int n = tbase + (unsigned int)(q * HALF);
                const D2 o = {zv[0], zv[1]};
                char* zp = zcol + (size_t)(n * 8u);
                if (FULL || n + 1 < c1_32) band_store2<false>(zp, o.x, o.y);
                else if (n < c1_32) *(double*)zp = o.x;
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // (the slot as a constant of the type system: the policy of the store depends on it)
            band_slots<NP>([&](auto Q) {
                constexpr int q = decltype(Q)::value;
                band_forward_rows<CLS, LAG, FULL, OWN, band_z_nt<POL, q>>(q, xc, pend, rec, start, sp_a, sp_b, sp_ds, own1, nI, tab, etab, kt, tbase, zcol, c1_32);
            });
        }
        rec += PS; xcol += ldxb; zcol += ldzb;
    };
    int j = kb;
    for (; j + RING <= ke; j += RING) {
#pragma unroll
        for (int i = 0; i < RING; ++i) step(j + i, xr[i], xr[(i + PF) % RING]);
    }
#pragma unroll
    for (int i = 0; i < RING - 1; ++i)
        if (j + i < ke) step(j + i, xr[i], xr[(i + PF) % RING]);
}

// ---------------------------------------------------------------------------
// fused density pass: S (optional), sum_k log(dS_k/dx_k / sigma_k) and sum_k S_k^2 per row (TM:2569-2712)
// ---------------------------------------------------------------------------
// log(x): fdlibm's polynomial on the reduced argument, division by a Newton reciprocal (<= 2 ulp)
__device__ __forceinline__ double band_log(double x) {
    int e;
    double m = frexp(x, &e);                                  // [0.5, 1)
    const bool small = m < 0.70710678118654752440;
    m = small ? m * 2.0 : m;
    e = small ? e - 1 : e;
    const double f = m - 1.0;
    const double den = 2.0 + f;
    double rc = __builtin_amdgcn_rcp(den);
    rc = fma(fma(-den, rc, 1.0), rc, rc);
    rc = fma(fma(-den, rc, 1.0), rc, rc);
    const double q = f * rc;
    const double sq = fma(fma(-den, q, f), rc, q);
    const double z = sq * sq;
    const double w = z * z;
    const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
    const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01), 2.857142874366239149e-01),
                              6.666666666666735130e-01);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    const double dk = (double)e;
    double res = dk * 6.93147180369123816490e-01 - ((hfsq - (sq * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
    // (0, negative, NaN, inf by selects - the library call here would be inlined into the column loop; denormals are
    // handled by frexp itself: the kernels run with fp64 denormals on)
    res = x == 0.0 ? -INFINITY : res;
    res = x < 0.0 ? NAN : res;
    res = (x != x || x == INFINITY) ? x : res;
    return res;
}

// the spline and its derivative with respect to the local coordinate
__device__ __forceinline__ void band_spline_d(const double* tab, int nI, double sp_a, double sp_b, double sp_ds, double x, double& m, double& dm) {
    const int col = band_med3((int)fma(x, sp_b, sp_a), 0, nI - 1);
    const double* cp = (const double*)((const char*)tab + __umul24((unsigned int)col, TTM_U_TSTRIDE * 8));
    double c[12];
#pragma unroll
    for (int i = 0; i < 12; i += 2) { const D2 v = *(const D2*)(cp + i); c[i] = v.x; c[i + 1] = v.y; }
    const double s = fma(x, sp_ds, cp[12]);
    double a = c[11], da = 0.0;
#pragma unroll
    for (int i = 10; i >= 0; --i) {
        da = fma(da, s, a);
        a = fma(a, s, c[i]);
    }
    m = a; dm = da;
}

// The log-determinant is taken as the log of the PRODUCT of a row's derivatives, renormalised every BAND_LD_CHUNK = 2 columns
// (mantissa kept, binary exponent counted - round 5: every TWO columns; four tail derivatives of 1e-90 each - grid points far
// outside the samples of a monotone part that saturates - underflow a product of four where the reference's sum of logarithms
// is finite): ONE logarithm per row instead of one per evaluation; the uniform factors of the derivatives (2/h of every
// spline, 1/sigma_k) enter as one number per launch.
#define BAND_LD_CHUNK 2
#define BAND_UNI 256                                  /* components of a density pass, at most */
#define BAND_DENS_NS 4
template <int CLS, int LAG, bool WRITE_Z, bool OWN>
__global__ __launch_bounds__(BAND_CT) void k_band_density(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                          const double* __restrict__ X, int64_t ldx, int64_t N,
                                                          double* __restrict__ Z, int64_t ldz, double* __restrict__ logdet,
                                                          const double* __restrict__ sigma, double* __restrict__ sumsq,
                                                          int64_t rows_per_wg, int Bc) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    // (two rows per thread: the pass carries three more running values per row than the plain map and is bound by its
    // arithmetic, not by the column stream)
    // (four rows per thread without Z; with it the masked stores of every step copy leave registers for two - and so does the
    // own term: slope, the branch around a missing spline and the derivative formed per evaluation spill ~280 registers at four)
    constexpr bool SHORT = WRITE_Z || OWN;                // two rows per thread, two columns per trip of the column loop
    constexpr int NS = SHORT ? 2 : BAND_DENS_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    band_stage<false>(etab, g_band_etab, 2 * TTM_BAND_ET_N);      // (waited for with the first block's splines)
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int c1_32 = (unsigned int)c1;
    const int64_t ldxb = ldx * 8, ldzb = ldz * 8;
    // uniform part of the log-determinant: sum_k log(2 / h_k) - sum_k log(sigma_k): one logarithm per thread, summed in
    // component order by thread 0 (every thread taking all of them was a fifth of the launch).  OWN: dS_k/dx_k =
    // dm 2 / h_k + own1 has no uniform factor - the 2 / h_k are applied per evaluation, as k_band_few does
    __shared__ double s_uni[BAND_UNI];
    double luni;
    {
        const int ncomp = k1 - k0;
        for (int k = tid; k < ncomp; k += CT) {
            double v = OWN ? 0.0 : band_log(P[(int64_t)(k0 + k + LAG) * PS + 4]);
            if (sigma) v -= band_log(sigma[k]);
            s_uni[k] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            for (int k = 0; k < ncomp; ++k) acc += s_uni[k];
            s_uni[0] = acc;
        }
        __syncthreads();
        luni = s_uni[0];
    }
    for (int tile = 0; tile < ntile; ++tile) {
        const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = tbase + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        // log det = log of the PRODUCT of the row's derivatives: every BAND_LD_CHUNK columns the product is renormalised
        // (mantissa kept, exponent counted: two instructions where a logarithm takes 35), ONE logarithm per row at the end.
        // dmin: the smallest derivative of the row - a negative one makes the row NaN as the reference's log does (two of
        // them would cancel in the product)
        double ss[NS], prod[NS], dmin[NS];
        int pexp[NS];
#pragma unroll
        for (int e = 0; e < NS; ++e) { ss[e] = 0.0; prod[e] = 1.0; dmin[e] = 0.0; pexp[e] = 0; }
        double pend[NS][LAG];
        for (int kb = k0; kb < k1; kb += Bc) {
            const int ke = kb + Bc < k1 ? kb + Bc : k1;
            __syncthreads();
            int tab0;
            {
                cint_p rb = (cint_p)(P + (int64_t)(kb + LAG) * PS), re = (cint_p)(P + (int64_t)(ke - 1 + LAG) * PS);
                tab0 = rb[11];
                const int n = re[11] + TTM_U_TSTRIDE * re[10] - tab0;
                band_stage(tabs, U_ + tab0, n);
            }
            __syncthreads();
            const int colb = kcol0 + (kb - k0);
            if (kb == k0 || true) {
#pragma unroll
                for (int l = 0; l < LAG; ++l) {
                    const double s0 = P[(int64_t)(kb + l) * PS];
#pragma unroll
                    for (int e = 0; e < NS; ++e) pend[e][l] = s0;
                }
                if (colb > 0) {
                    for (int i = 0; i < LAG; ++i) {
                        const int cc = colb - LAG + i;
                        cdbl_p rec = P + (int64_t)(kb + i) * PS;
                        const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                        for (int q = 0; q < NP; ++q) {
                            D2 xv = *(const D2*)(col + roff[q]);
                            if (cc < 0) { xv.x = 0.0; xv.y = 0.0; }
                            band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.x, band_expq(etab, xv.x, kt), pend[2 * q]);
                            band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.y, band_expq(etab, xv.y, kt), pend[2 * q + 1]);
                        }
                    }
                }
            }
            const char* xcol = (const char*)X + (int64_t)colb * ldxb;
            char* zcol = WRITE_Z ? (char*)Z + (int64_t)(kb - k0) * ldzb : nullptr;
            cdbl_p rec = P + (int64_t)(kb + LAG) * PS;
            D2 xa[NP], xb[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) xa[q] = band_load2(xcol + roff[q]);
            auto step = [&](int j, const D2 (&xc)[NP], D2 (&xn)[NP]) {
                {
                    const char* xnext = j + 1 < ke ? xcol + ldxb : xcol;
#pragma unroll
                    for (int q = 0; q < NP; ++q) xn[q] = band_load2(xnext + roff[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
                const double start = rec[0], sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4];
                const double own1 = OWN ? rec[7] : 0.0;
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];
                const double* tab = tabs + (ri[11] - tab0);
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    double zv[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int e = 2 * q + h;
                        const double x = h ? xc[q].y : xc[q].x;
                        double m = 0.0, dm = 0.0;
                        if (!OWN || nI > 0) band_spline_d(tab, nI, sp_a, sp_b, sp_ds, x, m, dm);
                        const double E = band_expq(etab, x, kt);
                        zv[h] = OWN ? fma(own1, x, pend[e][0] + m) : pend[e][0] + m;
                        if (OWN) dm = fma(dm, sp_ds, fma(x, 0.0, own1));      // dS_k/dx_k (x 0: a NaN / infinite sample stays NaN)
                        ss[e] = fma(zv[h], zv[h], ss[e]);
                        prod[e] *= dm;
                        dmin[e] = fmin(dmin[e], dm);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, start, x, E, pend[e]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (WRITE_Z) {
                        const unsigned int n = tbase + (unsigned int)(q * HALF);
                        char* zp = zcol + (size_t)(n * 8u);
                        if (n + 1 < c1_32) band_store2<false>(zp, zv[0], zv[1]);
                        else if (n < c1_32) *(double*)zp = zv[0];
                    }
                }
                if (SHORT && (((j - k0) & (BAND_LD_CHUNK - 1)) == BAND_LD_CHUNK - 1)) {
#pragma unroll
                    for (int e = 0; e < NS; ++e) { int ex; prod[e] = frexp(prod[e], &ex); pexp[e] += ex; }
                }
                rec += PS; xcol += ldxb;
                if (WRITE_Z) zcol += ldzb;
            };
            // four columns at a time, then ONE place where the chunk's products go through the logarithm (inside the step the
            // four inlined logarithms of every step copy cost the registers of two rows)
            auto flush_ld = [&]() {
#pragma unroll
                for (int e = 0; e < NS; ++e) { int ex; prod[e] = frexp(prod[e], &ex); pexp[e] += ex; }
            };
            int j = kb;
            if (SHORT) {                                      // (fewer step copies: two columns at a time)
                for (; j + 1 < ke; j += 2) {
                    step(j, xa, xb);
                    step(j + 1, xb, xa);
                }
            } else {
                for (; j + 3 < ke; j += 4) {
                    step(j, xa, xb);
                    step(j + 1, xb, xa);
                    flush_ld();
                    step(j + 2, xa, xb);
                    step(j + 3, xb, xa);
                    flush_ld();
                }
                for (; j + 1 < ke; j += 2) {
                    step(j, xa, xb);
                    step(j + 1, xb, xa);
                    flush_ld();
                }
            }
            if (j < ke) step(j, xa, xb);
            flush_ld();
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const unsigned int n = tbase + (unsigned int)(q * HALF);
            if (logdet) {
                double lv[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int e = 2 * q + h;
                    lv[h] = fma((double)pexp[e], 6.93147180559945286e-01, band_log(prod[e])) + luni;
                    lv[h] = dmin[e] < 0.0 ? NAN : lv[h];
                }
                if (n + 1 < c1_32) band_store2<false>((char*)(logdet + n), lv[0], lv[1]);
                else if (n < c1_32) logdet[n] = lv[0];
            }
            if (sumsq) {
                if (n + 1 < c1_32) band_store2<false>((char*)(sumsq + n), ss[2 * q], ss[2 * q + 1]);
                else if (n < c1_32) sumsq[n] = ss[2 * q];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// log-determinant only (TM:2569-2712: sum_k log(dS_k/dx_k / sigma_k) per row, no map values): what the pullback /
// pushforward densities take on the raw samples (the reference evaluates its derivative basis on un-standardised x).
// dS_k/dx_k of a separable component is a function of x_k ALONE - the derivative of its special-term spline (+ the slope of
// a linear own term) - so the pass needs no running sums, no exp(-x^2/4), no pushes: per evaluation the spline's column
// (fma, cvt, med3, mad), its coefficients (six 16-byte LDS reads + the column offset), 21 FMAs for the derivative of the
// degree-11 local polynomial, one multiplication into the row's running product.  29 vector instructions (the fused
// density pass k_band_density: 65), bound by the LDS gathers (104 bytes per row and column) and the column stream.
// The product is renormalised every TWO columns (mantissa kept, binary exponent counted): derivatives of 1e-150 - grid
// points far outside the samples of a map whose monotone part saturates - cannot underflow it; ONE logarithm per row.
// The uniform factors (2/h_k of a spline without a linear term beside it, 1/sigma_k) enter once per launch.
// LDS: [splines of a block of components, as they stand in the U section]
// ---------------------------------------------------------------------------
__device__ __forceinline__ double band_spline_dd(const double* tab, int nI, double sp_a, double sp_b, double sp_ds, double x) {
    const int col = band_med3((int)fma(x, sp_b, sp_a), 0, nI - 1);
    const double* cp = (const double*)((const char*)tab + __umul24((unsigned int)col, TTM_U_TSTRIDE * 8));
    double c[12];
#pragma unroll
    for (int i = 0; i < 12; i += 2) { const D2 v = *(const D2*)(cp + i); c[i] = v.x; c[i + 1] = v.y; }
    // (c[0] is not part of the derivative; left unused, its half of the first 16-byte read is dropped and the remaining
    // coefficients are re-paired (c1, c2), (c3, c4) ... as ds_read2_b64 - half the rate of ds_read_b128 and banked modulo 32:
    // 36 % of the LDS cycles were bank conflicts.  The empty statement keeps the six aligned 16-byte reads.)
    asm volatile("" :: "v"(c[0]));
    const double s = fma(x, sp_ds, cp[12]);
    double a = c[11], da = 0.0;
#pragma unroll
    for (int i = 10; i >= 1; --i) {
        da = fma(da, s, a);
        a = fma(a, s, c[i]);
    }
    return fma(da, s, a);
}

#define BAND_LD_PF 3
template <int LAG, int NS>
__global__ __launch_bounds__(BAND_CT) void k_band_logdet(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0, int ps,
                                                         const double* __restrict__ X, int64_t ldx, int64_t N,
                                                         double* __restrict__ logdet, const double* __restrict__ sigma,
                                                         int64_t rows_per_wg, int Bc) {
    constexpr int NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    double* tabs = g_lds;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    cdbl_p P = (cdbl_p)(U_ + p_off);
    const int64_t PS = ps;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int c1_32 = (unsigned int)c1;
    const int64_t ldxb = ldx * 8;
    // uniform part: sum_k [log(2 / h_k) for a spline without a linear term beside it] - sum_k log(sigma_k), one logarithm
    // per thread, summed in component order by thread 0
    __shared__ double s_uni[BAND_UNI];
    double luni;
    {
        const int ncomp = k1 - k0;
        for (int k = tid; k < ncomp; k += CT) {
            cdbl_p rec = P + (int64_t)(k0 + k + LAG) * PS;
            cint_p ri = (cint_p)rec;
            double v = (ri[10] > 0 && rec[7] == 0.0) ? band_log(rec[4]) : 0.0;
            if (sigma) v -= band_log(sigma[k]);
            s_uni[k] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            for (int k = 0; k < ncomp; ++k) acc += s_uni[k];
            s_uni[0] = acc;
        }
        __syncthreads();
        luni = s_uni[0];
    }
    for (int kb = k0; kb < k1; kb += Bc) {
        const int ke = kb + Bc < k1 ? kb + Bc : k1;
        const bool first = kb == k0, last = ke == k1;
        __syncthreads();
        int tab0;
        {
            // (components without special terms have no spline: the block's splines lie between the first and the last that has one)
            int tb = -1, te = 0;
            for (int k = kb; k < ke; ++k) {
                cint_p r = (cint_p)(P + (int64_t)(k + LAG) * PS);
                if (r[10] > 0) { if (tb < 0) tb = r[11]; te = r[11] + TTM_U_TSTRIDE * r[10]; }
            }
            tab0 = tb < 0 ? 0 : tb;
            const int n = tb < 0 ? 0 : te - tb;
            band_stage(tabs, U_ + tab0, n);
        }
        __syncthreads();
        for (int tile = 0; tile < ntile; ++tile) {
            const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
            unsigned int roff[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                unsigned int n = tbase + (unsigned int)(q * HALF);
                n = n < last_pair ? n : last_pair;
                roff[q] = n * 8u;
            }
            double prod[NS], dmin[NS];
            int pexp[NS];
#pragma unroll
            for (int e = 0; e < NS; ++e) { prod[e] = 1.0; dmin[e] = 0.0; pexp[e] = 0; }
            const char* xcol = (const char*)X + (int64_t)(kcol0 + (kb - k0)) * ldxb;
            cdbl_p rec = P + (int64_t)(kb + LAG) * PS;
            // The column stream is latency bound (a step of a SIMD's four waves is shorter than a loaded memory round trip): the
            // column of step j + PF is requested at the top of step j, PF + 1 register sets take turns (steps are issued
            // PF + 1 at a time with the roles rotated: no set is ever copied).  This pass has the registers for PF = 3
            // (six 1 KB loads in flight per wave: 96 KB per CU).
            constexpr int PF = BAND_LD_PF, RING = PF + 1;
            D2 xr[RING][NP];
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const char* xc0 = xcol + (int64_t)(kb + i < ke ? i : 0) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) xr[i][q] = band_load2(xc0 + roff[q]);
            }
            auto step = [&](int j, const D2 (&xc)[NP], D2 (&xn)[NP]) {
                {
                    const char* xnext = j + PF < ke ? xcol + PF * ldxb : xcol;       // (past the block: a harmless re-read)
#pragma unroll
                    for (int q = 0; q < NP; ++q) xn[q] = band_load2(xnext + roff[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
                const double sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4], own1 = rec[7];
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];
                const double* tab = tabs + (ri[11] - tab0);
                if (nI > 0 && own1 == 0.0) {
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int e = 2 * q + h;
                            const double dm = band_spline_dd(tab, nI, sp_a, sp_b, sp_ds, h ? xc[q].y : xc[q].x);
                            prod[e] *= dm;
                            dmin[e] = fmin(dmin[e], dm);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int e = 2 * q + h;
                            const double x = h ? xc[q].y : xc[q].x;
                            const double dm = nI > 0 ? band_spline_dd(tab, nI, sp_a, sp_b, sp_ds, x) : 0.0;
                            const double dx = fma(dm, sp_ds, fma(x, 0.0, own1));     // (x 0: a NaN / infinite sample stays NaN)
                            prod[e] *= dx;
                            dmin[e] = fmin(dmin[e], dx);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                rec += PS; xcol += ldxb;
            };
            auto flush = [&]() {
#pragma unroll
                for (int e = 0; e < NS; ++e) { int ex; prod[e] = frexp(prod[e], &ex); pexp[e] += ex; }
            };
            int j = kb;
            for (; j + RING <= ke; j += RING) {
#pragma unroll
                for (int i = 0; i < RING; ++i) {
                    step(j + i, xr[i], xr[(i + PF) % RING]);
                    if (i & 1) flush();
                }
                if (RING & 1) flush();
            }
#pragma unroll
            for (int i = 0; i < RING - 1; ++i) {
                if (j + i < ke) {
                    step(j + i, xr[i], xr[(i + PF) % RING]);
                    if (i & 1) flush();
                }
            }
            flush();
            // a block's share of the row's log-determinant: kept in the output between the blocks (one block at C5)
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const unsigned int n = tbase + (unsigned int)(q * HALF);
                double lv[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int e = 2 * q + h;
                    lv[h] = fma((double)pexp[e], 6.93147180559945286e-01, band_log(prod[e]));
                    lv[h] = dmin[e] < 0.0 ? NAN : lv[h];
                    if (last) lv[h] += luni;
                }
                if (!first) {
                    if (n + 1 < c1_32) { const D2 o = *(const D2*)(logdet + n); lv[0] += o.x; lv[1] += o.y; }
                    else if (n < c1_32) lv[0] += logdet[n];
                }
                if (n + 1 < c1_32) band_store2<false>((char*)(logdet + n), lv[0], lv[1]);
                else if (n < c1_32) logdet[n] = lv[0];
            }
        }
    }
}

// LDS: [E table: 2 x 801 | splines of the block's components, as they stand in the U section]
// POL: the cache policy of the column streams (band_store2 ff.; the host's choice: ttm_band_policy.h)
template <int CLS, int LAG, bool OWN, int POL = 0>
__global__ __launch_bounds__(BAND_CT) void k_band_forward(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                          const double* __restrict__ X, int64_t ldx, int64_t N,
                                                          double* __restrict__ Z, int64_t ldz, int64_t rows_per_wg, int Bc) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    band_stage<false>(etab, g_band_etab, 2 * TTM_BAND_ET_N);      // (waited for with the first block's splines)
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);      // first row of the last readable pair
    const unsigned int c1_32 = (unsigned int)c1;
    const int64_t ldxb = ldx * 8, ldzb = ldz * 8;

    for (int kb = k0; kb < k1; kb += Bc) {
        const int ke = kb + Bc < k1 ? kb + Bc : k1;
        __syncthreads();                                      // every wave is done with the previous block's splines
        int tab0;
        {
            cint_p rb = (cint_p)(P + (int64_t)(kb + LAG) * PS), re = (cint_p)(P + (int64_t)(ke - 1 + LAG) * PS);
            tab0 = rb[11];
            const int n = re[11] + TTM_U_TSTRIDE * re[10] - tab0;           // doubles (even)
            band_stage(tabs, U_ + tab0, n);
        }
        __syncthreads();
        const int colb = kcol0 + (kb - k0);                   // column of component kb
        for (int tile = 0; tile < ntile; ++tile) {
            const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
            const bool full = c0 + (int64_t)(tile + 1) * ROWS <= c1;
            unsigned int roff[NP];                            // byte offsets of this thread's pairs within a column (clamped: loads)
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                unsigned int n = tbase + (unsigned int)(q * HALF);
                n = n < last_pair ? n : last_pair;
                roff[q] = n * 8u;
            }
            // running sums of the components kb .. kb + LAG - 1 at this point of the sweep
            double pend[NS][LAG];
#pragma unroll
            for (int l = 0; l < LAG; ++l) {
                const double s = P[(int64_t)(kb + l) * PS];
#pragma unroll
                for (int e = 0; e < NS; ++e) pend[e][l] = s;
            }
            if (colb > 0) {
                // the LAG columns in front of the block, pushed without being evaluated (a column that does not exist has
                // an all-zero record: with x = 0, E = 1 its step only shifts the sums)
                for (int i = 0; i < LAG; ++i) {
                    const int cc = colb - LAG + i;
                    cdbl_p rec = P + (int64_t)(kb + i) * PS;
                    const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        D2 xv = *(const D2*)(col + roff[q]);
                        if (cc < 0) { xv.x = 0.0; xv.y = 0.0; }
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.x, band_expq(etab, xv.x, kt), pend[2 * q]);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.y, band_expq(etab, xv.y, kt), pend[2 * q + 1]);
                    }
                }
            }
            const char* xcol = (const char*)X + (int64_t)colb * ldxb;
            char* zcol = (char*)Z + (int64_t)(kb - k0) * ldzb;
            if (full) band_forward_tile<CLS, LAG, true, OWN, POL>(P, kt, etab, tabs, tab0, kb, ke, xcol, ldxb, zcol, ldzb, tbase, roff, c1_32, pend);
            else band_forward_tile<CLS, LAG, false, OWN, POL>(P, kt, etab, tabs, tab0, kb, ke, xcol, ldxb, zcol, ldzb, tbase, roff, c1_32, pend);
        }
    }
}

// ---------------------------------------------------------------------------
// maps of a few components (at most TTM_P_FEW_D: the spiral / temperature / banana examples, the filter and smoother
// blocks): a launch is a handful of microseconds, so what counts is the chain of memory round trips in front of the
// first store.  Here it is ONE: the E table, every spline and ALL columns of the tile are requested together (tables
// first - the counter of outstanding loads retires in order), the tables go to LDS while the columns travel, then the
// columns are walked in registers.  Same arithmetic per row as k_band_forward / k_band_density.
// DENS: also sum_k log(dS_k/dx_k / sigma_k) and sum_k S_k^2 per row (Z optional)
// ---------------------------------------------------------------------------
#define BAND_FEW_NS 2                                 /* rows per thread and tile of the few-component kernels */
#define BAND_FEW_TAB (4 * BAND_CT)                    /* doubles of splines a launch can stage (two 16-byte loads per thread) */
// LAG: groups per push record (u_p_lag); LAGE <= LAG: how far back a group of the sweep reaches; PLAIN: some group has
// plain polynomial terms
template <int CLS, int LAG, int LAGE, bool PLAIN, bool DENS>
__global__ __launch_bounds__(BAND_CT) void k_band_few(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                      const double* __restrict__ X, int64_t ldx, int64_t N,
                                                      double* __restrict__ Z, int64_t ldz, double* __restrict__ logdet,
                                                      const double* __restrict__ sigma, double* __restrict__ sumsq, int ntiles,
                                                      int tab0, int ntab) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), GP = cls_gp(CLS), PS = rec_stride(CLS, LAG);
    // two rows (one 16-byte pair) per thread and tile: with tiles of 2048 rows even half a million rows reach every CU;
    // the columns of a workgroup's next tile are requested before the current one is evaluated
    constexpr int NS = BAND_FEW_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT, FD = TTM_P_FEW_D;
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int nc = k1 - k0;
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int N32 = (unsigned int)N;
    const int64_t ldxb = ldx * 8, ldzb = ldz * 8;
    // tables (tab0: offset of the first spline in the U section, ntab doubles - even, <= BAND_FEW_TAB: from the host, which
    // knows them, so the request does not wait for a record): requested now, written to LDS after the first tile's columns
    // have been requested
    const D2 ev = *(const D2*)(g_band_etab + 2 * min(tid, TTM_BAND_ET_N - 1));
    D2 sv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) sv[r] = *(const D2*)(U_ + tab0 + min(2 * tid + r * 2 * CT, ntab - 2));
    __builtin_amdgcn_sched_barrier(0);
    double luni = 0.0;
    bool staged = false;
    // every column of a tile: the LAGE columns in front of the first component (conditioning columns; none: zeros) and the
    // components' own (clamped duplicates beyond the last: unconditional loads stay in flight together)
    auto request = [&](int tile, D2 (&xf)[LAGE][NP], D2 (&xin)[FD][NP]) {
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAGE; ++i) {
                const int cc = kcol0 - LAGE + i;
                const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) xf[i][q] = band_load2(col + roff[q]);
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            const char* col = (const char*)X + (int64_t)(kcol0 + min(j, nc - 1)) * ldxb;
#pragma unroll
            for (int q = 0; q < NP; ++q) xin[j][q] = band_load2(col + roff[q]);
        }
    };
    D2 xf[LAGE][NP], xin[FD][NP], xfn[LAGE][NP], xinn[FD][NP];
    if ((int)blockIdx.x < ntiles) request(blockIdx.x, xf, xin);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned int tbase = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        __builtin_amdgcn_sched_barrier(0);
        if (!staged) {
            if (tid < TTM_BAND_ET_N) *(D2*)(etab + 2 * tid) = ev;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = 2 * tid + r * 2 * CT;
                if (i < ntab) *(D2*)(tabs + i) = sv[r];
            }
            if (DENS && sigma) {
                // uniform part of the log-determinant: - sum_k log(sigma_k), in component order (the 2 / h_k of the splines
                // are applied per evaluation here: a component may have a linear term next to its spline, or no spline)
                for (int k = 0; k < nc; ++k) luni -= band_log(sigma[k]);
            }
            __syncthreads();
            staged = true;
        }
        // (the density pass has no registers to spare for a second set of columns: its next tile is requested after this one)
        const bool more = tile + (int)gridDim.x < ntiles;
        if (more && !DENS) request(tile + gridDim.x, xfn, xinn);
        __builtin_amdgcn_sched_barrier(0);
        double pend[NS][LAGE];
#pragma unroll
        for (int l = 0; l < LAGE; ++l) {
            const double s0 = P[(int64_t)(k0 + l) * PS];
#pragma unroll
            for (int e = 0; e < NS; ++e) pend[e][l] = s0;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAGE; ++i) {
                // (record of the column LAGE - i in front of component k0; the chain it starts is component k0 + i's)
                const bool there = kcol0 - LAGE + i >= 0;
                cdbl_p rec = P + (int64_t)(k0 + LAG - LAGE + i) * PS;
                const double start = P[(int64_t)(k0 + i) * PS];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const double xa = there ? xf[i][q].x : 0.0, xb = there ? xf[i][q].y : 0.0;
                    band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xa, band_expq(etab, xa, kt), pend[2 * q]);
                    band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xb, band_expq(etab, xb, kt), pend[2 * q + 1]);
                }
            }
        }
        double ss[NS], prod[NS], dmin[NS];
        int pexp[NS];
#pragma unroll
        for (int e = 0; e < NS; ++e) { ss[e] = 0.0; prod[e] = 1.0; dmin[e] = 0.0; pexp[e] = 0; }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            if (DENS && j == 2 && nc > 2) {
                // the product of a row's derivatives is renormalised after two factors (mantissa kept, binary exponent counted):
                // derivatives of 1e-150 in every column - grid points far outside the samples of a monotone part that saturates -
                // would underflow a product of four where the reference's sum of logarithms is finite
#pragma unroll
                for (int e = 0; e < NS; ++e) { int ex; prod[e] = frexp(prod[e], &ex); pexp[e] = ex; }
            }
            if (j < nc) {
                cdbl_p rec = P + (int64_t)(k0 + j + LAG) * PS;
                const double start = P[(int64_t)(k0 + j + LAGE) * PS];        // (of the component LAGE columns on)
                const double sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4], own1 = rec[7];      // own1: slope of the component's linear term
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];                                                  // (0: no special terms, no spline)
                const double* tab = tabs + (ri[11] - tab0);
                char* zcol = (char*)Z + (int64_t)j * ldzb;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    double zv[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int e = 2 * q + h;
                        const double x = h ? xin[j][q].y : xin[j][q].x;
                        double m = 0.0, dm = 0.0;
                        if (nI > 0) {
                            if (DENS) band_spline_d(tab, nI, sp_a, sp_b, sp_ds, x, m, dm);
                            else m = band_spline(tab, nI, sp_a, sp_b, sp_ds, x);
                        }
                        const double E = band_expq(etab, x, kt);
                        zv[h] = fma(own1, x, pend[e][0] + m);
                        if (DENS) {
                            const double dx = fma(dm, sp_ds, own1);           // dS_k/dx_k in standardised units
                            ss[e] = fma(zv[h], zv[h], ss[e]);
                            prod[e] *= dx;
                            dmin[e] = fmin(dmin[e], dx);
                        }
                        band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, x, E, pend[e]);
                    }
                    if (!DENS || Z) {
                        const unsigned int n = tbase + (unsigned int)(q * HALF);
                        char* zp = zcol + (size_t)(n * 8u);
                        if (n + 1 < N32) band_store2<true>(zp, zv[0], zv[1]);
                        else if (n < N32) *(double*)zp = zv[0];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (DENS) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const unsigned int n = tbase + (unsigned int)(q * HALF);
                if (logdet) {
                    // (a negative derivative makes the row NaN, as the reference's log does: two would cancel in the product)
                    const double la = dmin[2 * q] < 0.0 ? NAN : fma((double)pexp[2 * q], 6.93147180559945286e-01, band_log(prod[2 * q])) + luni;
                    const double lb = dmin[2 * q + 1] < 0.0 ? NAN : fma((double)pexp[2 * q + 1], 6.93147180559945286e-01, band_log(prod[2 * q + 1])) + luni;
                    if (n + 1 < N32) band_store2<false>((char*)(logdet + n), la, lb);
                    else if (n < N32) logdet[n] = la;
                }
                if (sumsq) {
                    if (n + 1 < N32) band_store2<false>((char*)(sumsq + n), ss[2 * q], ss[2 * q + 1]);
                    else if (n < N32) sumsq[n] = ss[2 * q];
                }
            }
        }
        if (more && DENS) request(tile + gridDim.x, xf, xin);
        if (more && !DENS) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
#pragma unroll
                for (int i = 0; i < LAGE; ++i) xf[i][q] = xfn[i][q];
#pragma unroll
                for (int jj = 0; jj < FD; ++jj) xin[jj][q] = xinn[jj][q];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// table inverse (TM:3987-4084) in push form
// ---------------------------------------------------------------------------
// The resident-table machinery is that of k_inverse_rt (csrc/ttm_kernels.hip: blocks of components, windowed tables,
// 16-bit bucket index, the index kernel's bucket function bit for bit, outliers redone from the table in memory); the
// step is new: the nonmonotone offset of a component is the running sum pend[0] its predecessors pushed, the solved
// x_k is pushed on at once (exp(-x_k^2/4) from the located interval), and a step whose rows all lie inside the
// resident window - all but a handful per million - is ONE basic block.
// LDS (doubles): [tables: B x tab_slot | {E_i, y_i}: 2 x Weven]
// table slot: [wl, wh, bucket scale, bucket bias, int32 {entries per bucket at most, 0}, int32 {degenerate, 0} | xs: W
//              entries + 4 sentinels (+inf), rounded up to even | bucket index: nb + 1 uint16]
#define BAND_RT_KMAX 24                                /* components per block, at most (BAND_RT_HDR, band_bucket_params: ttm_band_image.h) */

// exp(-x^2/4) by the series (block boundaries, outliers): Cody-Waite reduction + degree-12 Taylor, <= 2 ulp
__device__ __forceinline__ double band_expq_series(double x) {
    const double y = fmax(-0.25 * (x * x), -800.0);
    const double k = rint(y * 1.4426950408889634);
    double r = fma(-k, 6.93147180369123816490e-01, y);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 2.08767569878681e-09;
    p = fma(p, r, 2.505210838544172e-08);
    p = fma(p, r, 2.755731922398589e-07);
    p = fma(p, r, 2.7557319223985893e-06);
    p = fma(p, r, 2.48015873015873e-05);
    p = fma(p, r, 0.0001984126984126984);
    p = fma(p, r, 0.001388888888888889);
    p = fma(p, r, 0.008333333333333333);
    p = fma(p, r, 0.041666666666666664);
    p = fma(p, r, 0.16666666666666666);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return fma(x, 0.0, ldexp(p, (int)k));
}

// LDS addresses as 32-bit pointers (a laundered generic pointer would be read through the flat path)
typedef const __attribute__((address_space(3))) char* lds_p;
__device__ __forceinline__ lds_p band_lds(const void* p) { return (lds_p)p; }
__device__ __forceinline__ double band_lds_f64(lds_p p) { return *(const __attribute__((address_space(3))) double*)p; }
// ... an 8-byte read the load/store optimiser cannot pair with its neighbour (ds_read2_b64 is served at a quarter of the
// rate of two ds_read_b64 and banks modulo 32)
__device__ __forceinline__ double band_lds_f64_single(lds_p p) {
    asm volatile("" : "+v"(p));
    return *(const __attribute__((address_space(3))) double*)p;
}
typedef double band_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ D2 band_lds_pair(lds_p p) {
    const band_v2 v = *(const __attribute__((address_space(3))) band_v2*)p;
    const D2 r = {v.x, v.y};
    return r;
}

// everything a tile needs to walk the columns [kb, ke) of a block
struct BandInvCtx {
    cdbl_p P, kt;
    const double* tabs;            // resident tables of the block
    lds_p etab1;                   // pairs {E_i, y_i}: entry i - 1 of the whole table at etab1 + 16 i
    const double* tab_x; const double* tmin; const double* tmax;
    int T, nb, tab_slot, w0, Weven, k0;
    double y0, ystep, ylast;
    int64_t ldzb, ldxb;
    unsigned int c1_32;
};

// The ring of resident tables (k_band_inverse_ring): step s of a workgroup's flat sequence (tile by tile, column by column)
// finds the image of its component in slot s mod R.  EVERY step copies ONE image by DMA - each wave one 1 KB piece, without a
// condition, so that the compiler's count of the loads in flight stays exact and the wait for the next column of z covers
// nothing else: the image of step s - G + R goes into the slot step s - G used.  The workgroup meets at a barrier every G
// steps, so that slot has been free since the last meeting; a piece requested before the last meeting has landed by the next
// one (counted wait: every step since put at least three vector-memory operations behind it), the barrier makes that true
// of every wave's piece, and the image is used at step s - G + R >= s + 2 G (R >= 3 G).  Past the last column the copies are
// harmless repeats.
struct BandRing {
    const char* src;               // this lane's 16 bytes inside the image of component k0
    unsigned int dst;              // where the wave's piece starts inside a slot (bytes)
    unsigned int tabs_lds;         // LDS address of slot 0
    unsigned int stride;           // bytes per image / slot
    int R, ncomp;
    int pos;                       // slot of the next step
    int tpos, tcomp;               // slot the next step refills, component whose image goes there
    int gcnt;                      // steps since the last meeting
};

// the images of the steps [0, n) into the slots [0, n) (in front of the first column: 16 bytes per lane and round)
__device__ __forceinline__ void band_ring_fill(const double* img, int ncomp, double* tabs, int tab_slot, int n) {
    const int U = tab_slot >> 1;                                              // 16-byte units per image
    const int total = n * U;
    for (int u0 = 0; u0 < total; u0 += BAND_CT) {
        const int u = u0 + (int)threadIdx.x;
        if (u < total) {
            const int t = u / U, o = u - t * U;
            band_dma16(img + (size_t)(t % ncomp) * tab_slot + 2 * o,
                       __builtin_amdgcn_readfirstlane(band_lds_addr(tabs) + (unsigned int)(u0 + ((int)threadIdx.x & ~63)) * 16u));
        }
    }
}

// POL = 1 (the ring kernel only): Z is loaded plainly in pair slot 0 and non-temporally in slot 1 (band_z_nt), X stored
// non-temporally; a partial tile's single rows, the DMA pieces and the outlier path's table reads stay plain
//
// ZD = 1 (the ring kernel beside POL = 1, FULL tiles only - the caller passes full = true): Z travels through LDS, two columns
// deep.  Every wave owns 2 KB of each of two column buffers (zq: the LDS address of its part of buffer 0; BAND_ZD_BUF bytes
// on, buffer 1); column c of the tile lives in buffer (c - kb) & 1.  Step j finds column j in registers, requests column
// j + 2 by two DMA instructions into the buffer column j came from, waits - a COUNTED wait - for column j + 1, requested a
// step ago, and reads it back: each lane the very 16-byte units its own DMA lanes wrote, so no other wave is involved and no
// barrier.  The caller has requested columns kb and kb + 1 and waited for them.  Past the last column the requests are
// harmless repeats, so that every step puts the same number of operations behind the one it waits for.
#define BAND_ZD_BUF (BAND_NS * BAND_CT * 8)          /* bytes of a column buffer: a tile's rows of one column */
static_assert(2 * BAND_ZD_BUF == BAND_ZDMA_LDS_BYTES, "ttm_band_policy.h counts the LDS of these two buffers");
template <int POL, int Q>
__device__ __forceinline__ void band_zd_request(const char* g, unsigned int lds_wave_base) {
    if (band_z_nt<POL, Q>) band_dma16_nt(g, lds_wave_base); else band_dma16(g, lds_wave_base);
}
//
// SL = 1 (the ring kernel only, ZD = 0): the images carry the slope of every interval (ttm_band_image.h, the slope layout) - the
// last phase of the search reads {E_lo, y_lo}, x_lo and the slope instead of forming the slope per row from x_hi and y_hi.
// The outlier path, which reads the table in memory, keeps forming it.
template <int CLS, int LAG, bool RING = false, int G = 0, int POL = 0, int ZD = 0, int SL = 0>
__device__ __forceinline__ void band_inverse_tile(const BandInvCtx& cx, bool full, int kb, int ke, const char* zcol, char* xcol, unsigned int tbase,
                                                  const unsigned int (&roff)[BAND_NS / 2], double (&pend)[BAND_NS][LAG],
                                                  const D2 (&zfirst)[BAND_NS / 2], bool have_first, BandRing* rg = nullptr, unsigned int zq = 0) {
    static_assert(ZD == 0 || (RING && POL == 1), "ZD = 1: the ring kernel under the resident policy");
    static_assert(SL == 0 || (RING && ZD == 0), "SL = 1: images with slopes, the ring kernel without the column buffers");
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, HALF = 2 * BAND_CT;
    cdbl_p rec = cx.P + (int64_t)(kb + LAG) * PS;
    cdbl_p kt = cx.kt;
    const double* slot = RING ? cx.tabs + (size_t)rg->pos * cx.tab_slot : cx.tabs;
    const double ystep = cx.ystep;
    const int nb1 = cx.nb - 1;
    D2 za[NP], zb[NP];
    // (ZD) this lane's unit of the wave's part of buffer 0, formed where it is used: three instructions the compiler cannot hoist.
    // Kept across the step it is one VGPR too many - spilled, and its reload, a vector-memory load the compiler counts, put
    // a wait in front of the read-back that drained the column requested a moment before
    auto zrd = [&]() {
        unsigned int a;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshl_add_u32 %0, %0, 4, %1" : "=&v"(a) : "s"(zq));
        return (lds_p)(uintptr_t)a;
    };
    if (ZD) {                                                 // (column kb has landed in buffer 0: the caller waited)
#pragma unroll
        for (int q = 0; q < NP; ++q) za[q] = band_lds_pair(zrd() + q * 1024);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else if (have_first) {                                         // (the chunk's first tile: requested before the block's tables)
#pragma unroll
        for (int q = 0; q < NP; ++q) za[q] = zfirst[q];
    } else {
        band_slots<NP>([&](auto Q) { constexpr int q = decltype(Q)::value; za[q] = band_load2<band_z_nt<POL, q>>(zcol + roff[q]); });
    }
    // interp1d slope form (TM:4062-4065) in the located interval and exp(-x^2/4) = E[i-1] exp(w), w = -delta (y_lo + x) / 4
    // from_image (std::true_type, SL only): the fourth argument IS the interval's slope as the image carries it and x_hi is not read;
    // std::false_type: it is y_hi and the slope is formed here.  One body, so that both forms share the series below to the letter.
    auto interp = [&](auto from_image, double y_lo, double y_hi_or_slope, double x_lo, double x_hi, double e_lo, double tgt, double& rr, double& ee) {
        // (the slope with the tie at a flat start: band_interval_slope; the abscissae are np.linspace's to the bit: include/ttm.h)
        const double slope = decltype(from_image)::value ? y_hi_or_slope : band_interval_slope(x_lo, x_hi, y_lo, y_hi_or_slope);
        const double delta = slope * (tgt - x_lo);
        rr = delta + y_lo;
        const double w = (delta * -0.25) * (y_lo + rr);
        double p = fma(kt[0], w, kt[1]);
        p = fma(p, w, kt[2]);
        p = fma(p, w, kt[3]);
        p = fma(p, w, kt[4]);
        p = fma(p, w, kt[5]);
        p = fma(p, w, 1.0);
        p = fma(p, w, 1.0);
        ee = e_lo * p;
    };
    auto step = [&](int j, const D2 (&zc)[NP], D2 (&zn)[NP], int par) {  // par: (j - kb) & 1 (ZD)
        if (ZD) {
            // column j + 2 into the buffer column j was read from (the reads have retired: lgkmcnt(0) at the end of the last step)
            const char* zreq = zcol + (j + 2 < ke ? 2 * cx.ldzb : j + 1 < ke ? cx.ldzb : 0);
            band_slots<NP>([&](auto Q) {
                constexpr int q = decltype(Q)::value;
                band_zd_request<POL, q>(zreq + roff[q], zq + (unsigned int)(par * BAND_ZD_BUF + q * 1024));
            });
        } else {
            const char* znext = j + 1 < ke ? zcol + cx.ldzb : zcol;           // (past the block: a harmless re-read)
            band_slots<NP>([&](auto Q) { constexpr int q = decltype(Q)::value; zn[q] = band_load2<band_z_nt<POL, q>>(znext + roff[q]); });
        }
        // the record of the step, requested NOW (left to itself the compiler loads the group coefficients where the pushes
        // use them - at the end of the step's dependent chain, a scalar-cache round trip on the critical path)
        double start = rec[1];
        double gc[LAG * (DB + 1 + DA)];
#pragma unroll
        for (int i = 0; i < LAG * (DB + 1 + DA); ++i) gc[i] = rec[TTM_P_HDR + i];
        asm volatile("" : "+s"(start));
#pragma unroll
        for (int i = 0; i < LAG * (DB + 1 + DA); ++i) asm volatile("" : "+s"(gc[i]));
        __builtin_amdgcn_sched_barrier(0);
        double wl, wh, scale, bias;
        { const D2 a = *(const D2*)slot; wl = a.x; wh = a.y; const D2 b = *(const D2*)(slot + 2); scale = b.x; bias = b.y; }
        const lds_p xsl = band_lds(slot + BAND_RT_HDR) - 8 * cx.w0;           // xs indexed by the entry's number in the whole table
        const lds_p bkl = band_lds(slot + BAND_RT_HDR + (SL ? 2 : 1) * cx.Weven);
        const bool deg = __builtin_amdgcn_readfirstlane(((const int*)slot)[10]) != 0;
        const int per = __builtin_amdgcn_readfirstlane(((const int*)slot)[8]);
        double traw[NS], tg[NS], r[NS], E[NS];
        unsigned long long outl = deg ? ~0ull : 0ull;
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            const double z = (e & 1) ? zc[e >> 1].y : zc[e >> 1].x;
            traw[e] = z - pend[e][0];
            tg[e] = fmin(fmax(traw[e], wl), wh);
            outl |= __builtin_amdgcn_ballot_w64(traw[e] != tg[e]);
        }
        if (RING && G > 0) {
            // the step's piece of an image (BandRing), behind the wait for this step's z (the ballot needs every row's target)
            band_dma16(rg->src + (size_t)rg->tcomp * rg->stride, rg->tabs_lds + (unsigned int)rg->tpos * rg->stride + rg->dst);
            if (++rg->tpos == rg->R) rg->tpos = 0;
            if (++rg->tcomp == rg->ncomp) rg->tcomp = 0;
        }
        if (ZD) {
            // column j + 1, requested at the top of the last step (or by the caller): behind its two requests stand that step's
            // piece and two stores and this step's two requests and piece - a full tile's step issues every one of them
            // unconditionally (an outlier path's loads in between only make the wait stricter)
            constexpr int PIECE = G > 0 ? 1 : 0, BEHIND = (PIECE + 2) + (2 + PIECE);   // last step: piece, stores; this one: requests, piece
            static_assert(BEHIND == (G > 0 ? 6 : 4), "the literal of the counted wait below");
            if (G > 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            const lds_p zr = zrd();
#pragma unroll
            for (int q = 0; q < NP; ++q) zn[q] = band_lds_pair(zr + ((par ^ 1) * BAND_ZD_BUF + q * 1024));
        }
        // the four rows in phases, so that their dependent LDS reads travel together: bucket -> the bucket's entries ->
        // the interval.  np.searchsorted(xs, target) (left) = entries in lower buckets + entries of the target's own
        // bucket that are below it (the bucket function is monotone: k_table_index); NC = entries compared (>= the most
        // any bucket of this table holds).  The target is clipped to the window's value range, so every read is resident
        // whatever the row (an outlier's result is replaced below).
        auto search = [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            int pos[NS];
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                const int bi = min((int)fma(tg[e], scale, bias), nb1);
                pos[e] = (int)*(const __attribute__((address_space(3))) unsigned short*)(bkl + 2 * bi);
            }
            double qv[NS][NC];
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                const lds_p q4 = xsl + 8 * pos[e];
                qv[e][0] = band_lds_f64(q4);
#pragma unroll
                for (int i = 1; i < NC; ++i) qv[e][i] = band_lds_f64_single(q4 + 8 * i);
            }
            D2 ey[NS];
            // (two whole bodies, not one with conditions inside: the SL = 0 body is the parent's text, and with it every SL = 0
            // instantiation keeps the parent's registers and spills - OPTLOG round 16 item 3)
            if constexpr (SL != 0) {
                double xlo[NS], slope[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
#pragma unroll
                    for (int i = 0; i < NC; ++i) pos[e] += qv[e][i] < tg[e] ? 1 : 0;
                    ey[e] = band_lds_pair(cx.etab1 + 16 * pos[e]);
                    const lds_p xp = xsl + 8 * pos[e];
                    xlo[e] = band_lds_f64(xp - 8);
                    slope[e] = band_lds_f64_single(xp + 8 * cx.Weven);         // (the slope of the interval below entry pos: indexed like xs)
                }
#pragma unroll
                for (int e = 0; e < NS; ++e) interp(std::true_type(), ey[e].y, slope[e], xlo[e], 0.0, ey[e].x, tg[e], r[e], E[e]);
            } else {
                double xlo[NS], xhi[NS], yhi[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
#pragma unroll
                    for (int i = 0; i < NC; ++i) pos[e] += qv[e][i] < tg[e] ? 1 : 0;
                    ey[e] = band_lds_pair(cx.etab1 + 16 * pos[e]);
                    yhi[e] = band_lds_f64_single(cx.etab1 + 16 * pos[e] + 24);    // (y of entry pos, from the pair behind; measured: a read off the pair's base register is slower)
                    const lds_p xp = xsl + 8 * pos[e];
                    xlo[e] = band_lds_f64(xp - 8);
                    xhi[e] = band_lds_f64_single(xp);
                }
#pragma unroll
                for (int e = 0; e < NS; ++e) interp(std::false_type(), ey[e].y, yhi[e], xlo[e], xhi[e], ey[e].x, tg[e], r[e], E[e]);
            }
        };
        if (per <= 2) search(std::integral_constant<int, 2>());
        else search(std::integral_constant<int, 4>());
        if (outl != 0) {
            // outliers (the tails of the table, beyond the window, NaN; every row of a degenerate table): clip as
            // TM:4074-4076, np.searchsorted (left) over the whole row in memory, the same interpolation
            const double* xg = cx.tab_x + (int64_t)(j - cx.k0) * cx.T;
            const double lo = cx.tmin[j - cx.k0], hi = cx.tmax[j - cx.k0];
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                if (deg || traw[e] != tg[e]) {
                    double t = traw[e];
                    const double cl = fmin(fmax(t, lo), hi);
                    t = t != t ? t : cl;                                      // a NaN target stays NaN
                    int a = 0, b = cx.T;
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (xg[mid] < t) a = mid + 1; else b = mid;
                    }
                    const int i = min(max(a, 1), cx.T - 1);
                    interp(std::false_type(), (double)(i - 1) * ystep + cx.y0, i == cx.T - 1 ? cx.ylast : (double)i * ystep + cx.y0, xg[i - 1], xg[i], band_expq_series((double)(i - 1) * ystep + cx.y0), t, r[e], E[e]);
                }
            }
        }
        // x_k is pushed on to the components that read it, and stored
#pragma unroll
        for (int e = 0; e < NS; ++e) band_push<DB, DA, LAG>(gc, start, r[e], E[e], pend[e]);
        if (full) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                band_store2<POL != 0>(xcol + (size_t)((tbase + (unsigned int)(q * HALF)) * 8u), r[2 * q], r[2 * q + 1]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const unsigned int n = tbase + (unsigned int)(q * HALF);
                const D2 o = {r[2 * q], r[2 * q + 1]};
                char* xp = xcol + (size_t)(n * 8u);
                if (n + 1 < cx.c1_32) { if (POL != 0) band_store2<true>(xp, o.x, o.y); else *(D2*)xp = o; }
                else if (n < cx.c1_32) *(double*)xp = o.x;
            }
        }
        rec += PS; slot += cx.tab_slot; zcol += cx.ldzb; xcol += cx.ldxb;
        if (ZD) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // (the next step's request overwrites what was just read)
        if (RING) {
            if (++rg->pos == rg->R) { rg->pos = 0; slot = cx.tabs; }
            if (G > 0 && ++rg->gcnt == G) {
                rg->gcnt = 0;
                // this wave's pieces from before the last meeting have landed: every step since put two column loads and a piece behind them
                // (ZD: five operations per step - two requests, the piece, two stores - and the last step's stores: 5 G + 2)
                static_assert(G == 0 || (3 * G - 2 == 10 && (2 + 1 + 2) * G + 2 == 22), "the literals of the counted waits below: 3 G - 2 and 5 G + 2");
                if (ZD) asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
                __syncthreads();
            }
        }
    };
    int j = kb;
    for (; j + 1 < ke; j += 2) {
        step(j, za, zb, 0);
        step(j + 1, zb, za, 1);
    }
    if (j < ke) step(j, za, zb, 0);
}

// KM: components per block, at most (what the table load is unrolled for: 4 for maps of a few components, BAND_RT_KMAX)
template <int CLS, int LAG, int KM>
__global__ __launch_bounds__(BAND_CT) void k_band_inverse(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                          const double* __restrict__ Z, int64_t ldz, double* X, int64_t ldx, int64_t N,
                                                          const double* __restrict__ tab_x, int T, double y0, double ystep, double ylast,
                                                          const double* __restrict__ tmin, const double* __restrict__ tmax,
                                                          const int* __restrict__ bkt, int nb, int tab_slot, int B, int64_t rows_per_wg,
                                                          int w0, int W) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    const int Weven = (W + 4 + 1) & ~1;
    double* tabs = g_lds;
    double* etab = tabs + (size_t)B * tab_slot;
    cdbl_p P = (cdbl_p)(U_ + p_off);
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const int64_t ldzb = ldz * 8, ldxb = ldx * 8;
    BandInvCtx cx;
    cx.P = P; cx.kt = (cdbl_p)g_band_taylor; cx.tabs = tabs;
    cx.etab1 = band_lds(etab) - 16 * w0 - 16;
    cx.tab_x = tab_x; cx.tmin = tmin; cx.tmax = tmax;
    cx.T = T; cx.nb = nb; cx.tab_slot = tab_slot; cx.w0 = w0; cx.Weven = Weven; cx.k0 = k0;
    cx.y0 = y0; cx.ystep = ystep; cx.ylast = ylast; cx.ldzb = ldzb; cx.ldxb = ldxb; cx.c1_32 = (unsigned int)c1;
    for (int i = tid; i < W; i += CT) {
        // E of grid point w0 + i and, next to it, that point's abscissa as np.linspace has it, to the bit (i * step + y0 in two
        // roundings, the last point forced): the interpolation reads y_lo with E and y_hi from the pair behind
        etab[2 * i] = band_expq_series(w0 + i == T - 1 ? ylast : (double)(w0 + i) * ystep + y0);
        etab[2 * i + 1] = w0 + i == T - 1 ? ylast : (double)(w0 + i) * ystep + y0;
    }
    double pend[NS][LAG];
#pragma unroll
    for (int e = 0; e < NS; ++e)
#pragma unroll
        for (int l = 0; l < LAG; ++l) pend[e][l] = 0.0;

    // Blocks of at most B components; odd workgroups take the short block first, so that neighbouring CUs reload their
    // tables at different times (a block switch stalls a CU for ~6 us; out of phase, the others use the bandwidth)
    int kfirst = B;
    if ((blockIdx.x & 1) && (k1 - k0) % B) kfirst = (k1 - k0) % B;
    for (int kb = k0, ke; kb < k1; kb = ke) {
        ke = kb + (kb == k0 ? kfirst : B);
        ke = ke < k1 ? ke : k1;
        const int nk = ke - kb;
        // the first column of z of the chunk's first tile is requested before the tables: one memory round trip instead of two
        // in a row (a block switch is a string of them; 8 us each before: profiles/r03_*)
        D2 zfirst[NP];
        {
            const char* zc0 = (const char*)Z + (int64_t)(kb - k0) * ldzb;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                unsigned int n = (unsigned int)c0 + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
                n = n < last_pair ? n : last_pair;
                zfirst[q] = band_load2(zc0 + (size_t)(n * 8u));
            }
        }
        __syncthreads();                                      // every wave is done with the previous block's tables
        // the tables of the block: every load of the block in flight at once (element i of every table by thread i; the
        // bucket indices sixteen bytes at a time), the search parameters next to them
        {
            constexpr int KMAX = KM;                          // components per block, at most (the host plans for it)
            double lo = 0.0, hi = 0.0;
            if (tid < nk) { lo = tmin[kb - k0 + tid]; hi = tmax[kb - k0 + tid]; }
            {
                double v[KMAX];
                const int i = tid < Weven ? tid : Weven - 1;  // (clamped, unconditional: all loads in flight together)
                const double* src = tab_x + (int64_t)(kb - k0) * T + w0 + min(i, W - 1);
#pragma unroll
                for (int u = 0; u < KMAX; ++u) v[u] = src[(int64_t)min(u, nk - 1) * T];
                // (stores unconditional too: a slot beyond the block's last table repeats that table's value - the clamped
                // load - into that table's slot; branches here would spill the values in flight)
#pragma unroll
                for (int u = 0; u < KMAX; ++u) tabs[(size_t)min(u, nk - 1) * tab_slot + BAND_RT_HDR + i] = i < W ? v[u] : INFINITY;
            }
            {
                constexpr int BR = (KMAX * 256 + CT - 1) / CT; // rounds of the bucket copy: a component's nb + 1 = 1024 int32 = 256 x 16 bytes
                int4 bv[BR];
#pragma unroll
                for (int rd = 0; rd < BR; ++rd) {
                    const int idx = rd * CT + tid, c = min(idx >> 8, nk - 1), w = idx & 255;
                    bv[rd] = *(const int4*)(bkt + (int64_t)(kb - k0 + c) * (nb + 1) + 4 * w);
                }
#pragma unroll
                for (int rd = 0; rd < BR; ++rd) {
                    const int idx = rd * CT + tid, c = min(idx >> 8, nk - 1), w = idx & 255;
                    unsigned short* bs = (unsigned short*)(tabs + (size_t)c * tab_slot + BAND_RT_HDR + Weven) + 4 * w;
                    const uint2 pk = {(unsigned int)(bv[rd].x & 0xffff) | ((unsigned int)bv[rd].y << 16),
                                      (unsigned int)(bv[rd].z & 0xffff) | ((unsigned int)bv[rd].w << 16)};
                    *(uint2*)bs = pk;
                }
            }
            if (tid < nk) {
                double* slot = tabs + (size_t)tid * tab_slot;
                double scale, bias;
                band_bucket_params(lo, hi, nb, scale, bias);
                slot[2] = scale; slot[3] = bias;
                ((int*)slot)[8] = 0; ((int*)slot)[9] = 0;
                slot[5] = 0.0;
            }
        }
        __syncthreads();
        // entries per bucket, at most; the value range [wl, wh] whose search stays inside the window (k_inverse_rt)
        for (int c = tid >> 6; c < nk; c += CT >> 6) {
            const unsigned short* bs = (const unsigned short*)(tabs + (size_t)c * tab_slot + BAND_RT_HDR + Weven);
            int per = 0;
            {                                                 // lane l: buckets 16 l .. 16 l + 15 from two 16-byte reads (nb + 1 = 1024 entries)
                const int l = tid & 63;
                const uint4 qa = *(const uint4*)(bs + 16 * l), qb = *(const uint4*)(bs + 16 * l + 8);
                const unsigned int nxt = l < 63 ? bs[16 * l + 16] : 0u;
                const unsigned int w[9] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w, nxt};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b0 = (int)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
                    const int b1 = (int)((w[(i + 1) >> 1] >> (16 * ((i + 1) & 1))) & 0xffffu);
                    if (16 * l + i < nb && b1 > w0 && b0 < w0 + W) per = max(per, b1 - b0);
                }
            }
            for (int o = 32; o > 0; o >>= 1) per = max(per, __shfl_xor(per, o));
            double* slot = tabs + (size_t)c * tab_slot;
            const int pm = max(per, 1);
            const bool deg = pm + 3 >= W || per > 4;                           // (more entries in a bucket than the resident search compares: every row by the outlier path)
            if ((tid & 63) == 0) {
                const double* xw = slot + BAND_RT_HDR;
                ((int*)slot)[8] = per;
                ((int*)slot)[10] = deg ? 1 : 0;
                slot[0] = deg ? xw[1] : xw[pm];
                slot[1] = deg ? xw[1] : xw[W - 2];
            }
            if (deg)
                for (int i = tid & 63; i <= nb; i += 64) const_cast<unsigned short*>(bs)[i] = (unsigned short)(w0 + 1);
        }
        __syncthreads();

        const int colb = kcol0 + (kb - k0);                   // column of component kb
        for (int tile = 0; tile < ntile; ++tile) {
            const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
            const bool full = c0 + (int64_t)(tile + 1) * ROWS <= c1;
            unsigned int roff[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                unsigned int n = tbase + (unsigned int)(q * HALF);
                n = n < last_pair ? n : last_pair;
                roff[q] = n * 8u;
            }
            if (!(ntile == 1 && kb > k0)) {
                // running sums at the block's first column from the LAG columns in front of it (conditioning columns, or
                // what the same thread stored in the block before); a chunk of ONE tile keeps them in registers instead
                for (int i = 0; i < LAG; ++i) {
                    const int cc = colb - LAG + i;
                    cdbl_p rec = P + (int64_t)(kb + i) * PS;
                    const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        D2 xv = {0.0, 0.0};
                        if (cc >= 0) xv = *(const D2*)(col + roff[q]);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[1], xv.x, cc >= 0 ? band_expq_series(xv.x) : 1.0, pend[2 * q]);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[1], xv.y, cc >= 0 ? band_expq_series(xv.y) : 1.0, pend[2 * q + 1]);
                    }
                }
            }
            const char* zcol = (const char*)Z + (int64_t)(kb - k0) * ldzb;
            char* xcol = (char*)X + (int64_t)colb * ldxb;
            band_inverse_tile<CLS, LAG>(cx, full, kb, ke, zcol, xcol, tbase, roff, pend, zfirst, tile == 0);
        }
    }
}

// ---------------------------------------------------------------------------
// k_band_inverse with the tables of a RING of components resident (BandRing, ttm_band_image.h): the images come ready-made
// from the kernel that built the tables and are copied into LDS by DMA - all R slots in front of the first column (one round
// trip: the first column of z is requested before them), then G at a time behind a barrier every G columns, two groups
// ahead of their use.  A tile walks ALL its columns in one go: the running sums never leave the registers, so the result of a
// row does not depend on the chunking (k_band_inverse re-reads LAG columns at a block boundary when a chunk has several tiles
// and takes their exp(-x^2/4) from the series there).  The step itself is band_inverse_tile, shared with k_band_inverse.
// POL: the cache policy of the column streams (band_inverse_tile; the host's choice: ttm_band_policy.h)
// ZD = 1: full tiles take Z through two column buffers in LDS behind the {E_i, y_i} pairs (band_inverse_tile; the ring has
// fewer slots: band_ring_plan_with), partial tiles run the code of ZD = 0
// SL = 1: the images carry the interval slopes (band_inverse_tile; the plan's choice: band_ring_plan) - beside ZD = 0 only
template <int CLS, int LAG, int G, int POL = 0, int ZD = 0, int SL = 0>
__global__ __launch_bounds__(BAND_CT) void k_band_inverse_ring(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                               const double* __restrict__ Z, int64_t ldz, double* X, int64_t ldx, int64_t N,
                                                               const double* __restrict__ tab_x, int T, double y0, double ystep, double ylast,
                                                               const double* __restrict__ tmin, const double* __restrict__ tmax,
                                                               const double* __restrict__ img, int nb, int tab_slot, int R,
                                                               int64_t rows_per_wg, int w0, int W) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    const int ncomp = k1 - k0;
    const int Weven = (W + 4 + 1) & ~1;
    double* tabs = g_lds;
    double* etab = tabs + (size_t)R * tab_slot;
    cdbl_p P = (cdbl_p)(U_ + p_off);
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const int64_t ldzb = ldz * 8, ldxb = ldx * 8;
    BandInvCtx cx;
    cx.P = P; cx.kt = (cdbl_p)g_band_taylor; cx.tabs = tabs;
    cx.etab1 = band_lds(etab) - 16 * w0 - 16;
    cx.tab_x = tab_x; cx.tmin = tmin; cx.tmax = tmax;
    cx.T = T; cx.nb = nb; cx.tab_slot = tab_slot; cx.w0 = w0; cx.Weven = Weven; cx.k0 = k0;
    cx.y0 = y0; cx.ystep = ystep; cx.ylast = ylast; cx.ldzb = ldzb; cx.ldxb = ldxb; cx.c1_32 = (unsigned int)c1;
    BandRing rg;
    {
        const int U = tab_slot >> 1, nw = (U + 63) >> 6;      // 16-byte units per image, waves that cover one
        const int piece = (tid >> 6) % nw;                    // (the other waves repeat a piece: the same bytes to the same place)
        const int start = 64 * piece < U - 64 ? 64 * piece : U - 64;
        rg.src = (const char*)img + (size_t)(start + (tid & 63)) * 16;
        rg.dst = __builtin_amdgcn_readfirstlane((unsigned int)start * 16u);
        rg.tabs_lds = band_lds_addr(tabs);
        rg.stride = (unsigned int)tab_slot * 8u;
        rg.R = R; rg.ncomp = ncomp; rg.pos = 0; rg.gcnt = 0;
        rg.tpos = G > 0 ? R - G : 0;
        rg.tcomp = G > 0 ? (R - G) % ncomp : 0;
    }
    // (ZD) this wave's 2 KB of column buffer 0, as an LDS address
    const unsigned int zq = ZD ? __builtin_amdgcn_readfirstlane(band_lds_addr(etab + 2 * Weven) + (unsigned int)(tid >> 6) * 2048u) : 0u;
    // a full tile's first two columns of z into the column buffers (ZD); the tile's rows are below N: no clamp
    auto zd_request2 = [&](int tile) {
        band_slots<NP>([&](auto Q) {
            constexpr int q = decltype(Q)::value;
            const unsigned int n = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
            const char* g = (const char*)Z + (size_t)(n * 8u);
            band_zd_request<POL, q>(g, zq + (unsigned int)(q * 1024));
            band_zd_request<POL, q>(k0 + 1 < k1 ? g + ldzb : g, zq + (unsigned int)(BAND_ZD_BUF + q * 1024));
        });
    };
    const bool zd0 = ZD != 0 && c0 + ROWS <= c1;               // (the first tile is full and takes z through LDS)
    // the first column of z of the first tile, then the images of the first R steps: one memory round trip
    D2 zfirst[NP];
    if (zd0) {
        zd_request2(0);
#pragma unroll
        for (int q = 0; q < NP; ++q) zfirst[q] = D2{0.0, 0.0};
    } else
    band_slots<NP>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        unsigned int n = (unsigned int)c0 + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
        n = n < last_pair ? n : last_pair;
        zfirst[q] = band_load2<band_z_nt<POL, q>>((const char*)Z + (size_t)(n * 8u));
    });
    band_ring_fill(img, ncomp, tabs, tab_slot, R);
    for (int i = tid; i < W; i += CT) {
        etab[2 * i] = band_expq_series(w0 + i == T - 1 ? ylast : (double)(w0 + i) * ystep + y0);
        etab[2 * i + 1] = w0 + i == T - 1 ? ylast : (double)(w0 + i) * ystep + y0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int tile = 0; tile < ntile; ++tile) {
        const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        const bool full = c0 + (int64_t)(tile + 1) * ROWS <= c1;
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = tbase + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        if (ZD && full && tile > 0) {
            // the last tile's trailing requests have landed before the buffers are requested into again; the wait for these two
            // columns stands behind the running sums below
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            zd_request2(tile);
        }
        // running sums at the first column from the LAG columns in front of it (conditioning columns, or nothing)
        double pend[NS][LAG];
#pragma unroll
        for (int e = 0; e < NS; ++e)
#pragma unroll
            for (int l = 0; l < LAG; ++l) pend[e][l] = 0.0;
        for (int i = 0; i < LAG; ++i) {
            const int cc = kcol0 - LAG + i;
            cdbl_p rec = P + (int64_t)(k0 + i) * PS;
            const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                D2 xv = {0.0, 0.0};
                if (cc >= 0) xv = *(const D2*)(col + roff[q]);
                band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[1], xv.x, cc >= 0 ? band_expq_series(xv.x) : 1.0, pend[2 * q]);
                band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[1], xv.y, cc >= 0 ? band_expq_series(xv.y) : 1.0, pend[2 * q + 1]);
            }
        }
        if (ZD && full) {
            if constexpr (ZD != 0) {
                if (tile > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                band_inverse_tile<CLS, LAG, true, G, POL, 1>(cx, true, k0, k1, (const char*)Z, (char*)X + (int64_t)kcol0 * ldxb, tbase, roff, pend, zfirst, false, &rg, zq);
            }
        } else
        band_inverse_tile<CLS, LAG, true, G, POL, 0, SL>(cx, full, k0, k1, (const char*)Z, (char*)X + (int64_t)kcol0 * ldxb, tbase, roff, pend, zfirst, tile == 0, &rg);
    }
}

// ---------------------------------------------------------------------------
// table inverse of maps with a few components: as k_band_few, ONE memory round trip in front of the first store - every
// table (whole, no window), every bucket index and all columns of the tile are requested together.  Tables of any shape:
// the bucket of a target is searched four ways at a time (three resident reads per phase, as many phases as the
// fullest bucket of the component needs: 1 up to 3 entries, 2 up to 15, 3 up to 63, 4 up to 255), where k_band_inverse
// compares up to four entries and sends fuller tables row by row to memory.
// LDS (doubles): [tables: nc x tab_slot | {E_i, y_i}: 2 x Weven];  table slot: [scale, bias, int32 {fullest bucket, 0},
// 0, 0, 0 (the entry "in front of the first") | xs: T entries + sentinels (+inf) up to Weven | bucket index: nb + 1 uint16]
// Needs nb + 1 = 1024 (one 16-byte load of bucket starts per thread) and T + 4 <= 1024 (entry i by thread i).
// ---------------------------------------------------------------------------
template <int CLS, int LAG, int LAGE, bool PLAIN>
__global__ __launch_bounds__(BAND_CT) void k_band_few_inverse(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                              const double* __restrict__ Z, int64_t ldz, double* X, int64_t ldx, int64_t N,
                                                              const double* __restrict__ tab_x, int T, double y0, double ystep, double ylast,
                                                              const double* __restrict__ tmin, const double* __restrict__ tmax,
                                                              const int* __restrict__ bkt, int nb, int tab_slot, int ntiles) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), GP = cls_gp(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_FEW_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT, FD = TTM_P_FEW_D, HDR = BAND_RT_HDR;
    extern __shared__ __align__(16) double g_lds[];
    const int tid = threadIdx.x;
    const int nc = k1 - k0;
    const int Weven = (T + 4 + 1) & ~1;
    double* tabs = g_lds;
    double* etab = tabs + (size_t)nc * tab_slot;
    const lds_p etab1 = band_lds(etab) - 16;                  // pair of entry i - 1 at etab1 + 16 i
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int N32 = (unsigned int)N;
    const int64_t ldzb = ldz * 8, ldxb = ldx * 8;
    const int nb1 = nb - 1;
    // tables and bucket starts: requested now (first: the counter of outstanding loads retires in order)
    double tv[FD];
    {
        const double* src = tab_x + min(tid, T - 1);
#pragma unroll
        for (int u = 0; u < FD; ++u) tv[u] = src[(int64_t)min(u, nc - 1) * T];
    }
    const int bc = min(tid >> 8, nc - 1), bw = tid & 255;     // this thread's four bucket starts: component, first bucket / 4
    const int4 bv = *(const int4*)(bkt + (int64_t)bc * (nb + 1) + 4 * bw);
    __builtin_amdgcn_sched_barrier(0);
    // interp1d slope form (TM:4062-4065) in the located interval and exp(-x^2/4) = E[i-1] exp(w), w = -delta (y_lo + x) / 4
    auto interp = [&](double y_lo, double y_hi, double x_lo, double x_hi, double e_lo, double tgt, double& rr, double& ee) {
        // (the slope with the tie at a flat start: band_interval_slope; the abscissae are np.linspace's to the bit: include/ttm.h)
        const double delta = band_interval_slope(x_lo, x_hi, y_lo, y_hi) * (tgt - x_lo);
        rr = delta + y_lo;
        const double w = (delta * -0.25) * (y_lo + rr);
        double p = fma(kt[0], w, kt[1]);
        p = fma(p, w, kt[2]);
        p = fma(p, w, kt[3]);
        p = fma(p, w, kt[4]);
        p = fma(p, w, kt[5]);
        p = fma(p, w, 1.0);
        p = fma(p, w, 1.0);
        ee = e_lo * p;
    };
    // every column of a tile: the conditioning columns in front of the first component (already in X) and z
    auto request = [&](int tile, D2 (&xf)[LAGE][NP], D2 (&zin)[FD][NP]) {
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAGE; ++i) {
                const int cc = kcol0 - LAGE + i;
                const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) xf[i][q] = band_load2(col + roff[q]);
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            const char* col = (const char*)Z + (int64_t)min(j, nc - 1) * ldzb;
#pragma unroll
            for (int q = 0; q < NP; ++q) zin[j][q] = band_load2(col + roff[q]);
        }
    };
    D2 xf[LAGE][NP], zin[FD][NP], xfn[LAGE][NP], zinn[FD][NP];
    if ((int)blockIdx.x < ntiles) request(blockIdx.x, xf, zin);
    bool staged = false;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned int tbase = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        __builtin_amdgcn_sched_barrier(0);
        if (!staged) {
            // E of grid point i and, next to it, that point's abscissa as np.linspace has it, to the bit (computed while the
            // loads travel)
            if (tid < T) {
                etab[2 * tid] = band_expq_series(tid == T - 1 ? ylast : (double)tid * ystep + y0);
                etab[2 * tid + 1] = tid == T - 1 ? ylast : (double)tid * ystep + y0;
            }
            if (tid < nc) {
                double* slot = tabs + (size_t)tid * tab_slot;
                double scale, bias;
                band_bucket_params(tmin[tid], tmax[tid], nb, scale, bias);
                slot[0] = scale; slot[1] = bias;
                ((int*)slot)[4] = 0; ((int*)slot)[5] = 0;
                slot[3] = 0.0; slot[4] = 0.0; slot[5] = 0.0;
            }
            // (stores unconditional: a slot beyond the last table repeats that table's value - the clamped load - into
            // that table's slot)
            if (tid < Weven) {
#pragma unroll
                for (int u = 0; u < FD; ++u) tabs[(size_t)min(u, nc - 1) * tab_slot + HDR + tid] = tid < T ? tv[u] : INFINITY;
            }
            {
                unsigned short* bs = (unsigned short*)(tabs + (size_t)bc * tab_slot + HDR + Weven) + 4 * bw;
                const uint2 pk = {(unsigned int)(bv.x & 0xffff) | ((unsigned int)bv.y << 16), (unsigned int)(bv.z & 0xffff) | ((unsigned int)bv.w << 16)};
                *(uint2*)bs = pk;
            }
            __syncthreads();
            // the fullest bucket of every table
            if ((tid >> 8) < nc) {
                const unsigned short* bs = (const unsigned short*)(tabs + (size_t)bc * tab_slot + HDR + Weven);
                const int b4 = bw < 255 ? (int)bs[4 * bw + 4] : bv.w;
                int per = max(bv.y - bv.x, max(bv.z - bv.y, bv.w - bv.z));
                per = max(per, b4 - bv.w);                    // (bucket nb does not exist: b4 = its start there, 0 entries)
                for (int o = 32; o > 0; o >>= 1) per = max(per, __shfl_xor(per, o));
                if ((tid & 63) == 0) atomicMax((int*)(tabs + (size_t)bc * tab_slot) + 4, per);
            }
            __syncthreads();
            staged = true;
        }
        const bool more = tile + (int)gridDim.x < ntiles;
        if (more) request(tile + gridDim.x, xfn, zinn);
        __builtin_amdgcn_sched_barrier(0);
        double pend[NS][LAGE];
#pragma unroll
        for (int l = 0; l < LAGE; ++l) {
            const double s0 = P[(int64_t)(k0 + l) * PS + 1];
#pragma unroll
            for (int e = 0; e < NS; ++e) pend[e][l] = s0;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAGE; ++i) {
                const bool there = kcol0 - LAGE + i >= 0;
                cdbl_p rec = P + (int64_t)(k0 + LAG - LAGE + i) * PS;
                const double start = P[(int64_t)(k0 + i) * PS + 1];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const double xa = there ? xf[i][q].x : 0.0, xb = there ? xf[i][q].y : 0.0;
                    band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xa, there ? band_expq_series(xa) : 1.0, pend[2 * q]);
                    band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xb, there ? band_expq_series(xb) : 1.0, pend[2 * q + 1]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            if (j < nc) {
                cdbl_p rec = P + (int64_t)(k0 + j + LAG) * PS;
                const double start = P[(int64_t)(k0 + j + LAGE) * PS + 1];
                const double* slot = tabs + (size_t)j * tab_slot;
                const double scale = slot[0], bias = slot[1];
                const int per = __builtin_amdgcn_readfirstlane(((const int*)slot)[4]);
                const int pm = max(per, 1);
                const bool deg = pm + 3 >= T || per > 255;
                const lds_p xsl = band_lds(slot + HDR);
                const lds_p bkl = band_lds(slot + HDR + Weven);
                const double wl = band_lds_f64(xsl + 8 * (deg ? 1 : pm)), wh = band_lds_f64(xsl + 8 * (deg ? 1 : T - 2));
                const int nph = per <= 3 ? 1 : per <= 15 ? 2 : per <= 63 ? 3 : 4;
                double traw[NS], tg[NS], r[NS], E[NS];
                unsigned long long outl = deg ? ~0ull : 0ull;
                int pos[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    const double z = (e & 1) ? zin[j][e >> 1].y : zin[j][e >> 1].x;
                    traw[e] = z - pend[e][0];
                    tg[e] = fmin(fmax(traw[e], wl), wh);
                    outl |= __builtin_amdgcn_ballot_w64(traw[e] != tg[e]);
                    const int bi = min((int)fma(tg[e], scale, bias), nb1);
                    pos[e] = (int)*(const __attribute__((address_space(3))) unsigned short*)(bkl + 2 * bi);
                }
                // np.searchsorted(xs, target) (left) = entries in lower buckets + entries of the target's own bucket below it
                // (the bucket function is monotone: k_table_index).  A phase of stride s tests the entries s, 2s, 3s on from
                // pos: every one below the target moves pos on by s; what is left are fewer than s candidates.
                for (int ph = 0, s = 1 << (2 * (nph - 1)); ph < nph; ++ph, s >>= 2) {
                    double qv[NS][3];
#pragma unroll
                    for (int e = 0; e < NS; ++e)
#pragma unroll
                        for (int i = 0; i < 3; ++i) qv[e][i] = band_lds_f64_single(xsl + 8 * min(pos[e] + (i + 1) * s - 1, T + 3));
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        int c = 0;
#pragma unroll
                        for (int i = 0; i < 3; ++i) c += qv[e][i] < tg[e] ? 1 : 0;
                        pos[e] += c * s;
                    }
                }
                {
                    D2 ey[NS];
                    double xlo[NS], xhi[NS], yhi[NS];
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        const int ps1 = band_med3(pos[e], 1, T - 1);          // (a flat start: the first interval, as the search in memory)
                        ey[e] = band_lds_pair(etab1 + 16 * ps1);
                        yhi[e] = band_lds_f64_single(etab1 + 16 * ps1 + 24);
                        const lds_p xp = xsl + 8 * ps1;
                        xlo[e] = band_lds_f64(xp - 8);
                        xhi[e] = band_lds_f64_single(xp);
                    }
#pragma unroll
                    for (int e = 0; e < NS; ++e) interp(ey[e].y, yhi[e], xlo[e], xhi[e], ey[e].x, tg[e], r[e], E[e]);
                }
                if (outl != 0) {
                    // outliers (the tails of the table, NaN; every row of a degenerate table): clip as TM:4074-4076,
                    // np.searchsorted (left) over the whole row in memory, the same interpolation
                    const double* xg = tab_x + (int64_t)j * T;
                    const double lo = tmin[j], hi = tmax[j];
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        if (deg || traw[e] != tg[e]) {
                            double t = traw[e];
                            const double cl = fmin(fmax(t, lo), hi);
                            t = t != t ? t : cl;                              // a NaN target stays NaN
                            int a = 0, b = T;
                            while (a < b) {
                                const int mid = (a + b) >> 1;
                                if (xg[mid] < t) a = mid + 1; else b = mid;
                            }
                            const int i = min(max(a, 1), T - 1);
                            interp((double)(i - 1) * ystep + y0, i == T - 1 ? ylast : (double)i * ystep + y0, xg[i - 1], xg[i], band_expq_series((double)(i - 1) * ystep + y0), t, r[e], E[e]);
                        }
                    }
                }
                // x_k is pushed on to the components that read it, and stored
#pragma unroll
                for (int e = 0; e < NS; ++e) band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, r[e], E[e], pend[e]);
                char* xcol = (char*)X + (int64_t)(kcol0 + j) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const unsigned int n = tbase + (unsigned int)(q * HALF);
                    char* xp = xcol + (size_t)(n * 8u);
                    if (n + 1 < N32) band_store2<true>(xp, r[2 * q], r[2 * q + 1]);
                    else if (n < N32) *(double*)xp = r[2 * q];
                }
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
#pragma unroll
                for (int i = 0; i < LAGE; ++i) xf[i][q] = xfn[i][q];
#pragma unroll
                for (int jj = 0; jj < FD; ++jj) zin[jj][q] = zinn[jj][q];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// forward map, (optionally) the density terms, and the table inverse of the image in ONE launch - what BASELINE configs[1]
// times as a step ("forward + inverse + pullback" of a map of a few components: two or three launches of ~10 us on 32 MB, each
// a launch floor and a memory round trip of its own).  A tile's columns are read once; z_k stays in registers between the
// forward sweep (k_band_few's arithmetic, statement for statement) and the inverse sweep (k_band_few_inverse's), which writes
// S^-1(S(x)) to Xr.  Same bits as the two (three) launches: tests/test_band.py::test_roundtrip_in_one_launch...
// LDS (doubles): [inverse tables: nc x tab_slot | {E_i, y_i}: 2 x Weven | forward exp table | forward splines: ntab]
// ---------------------------------------------------------------------------
template <int CLS, int LAG, int LAGE, bool PLAIN, bool DENS>
__global__ __launch_bounds__(BAND_CT) void k_band_few_roundtrip(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                                const double* __restrict__ X, int64_t ldx, int64_t N,
                                                                double* __restrict__ Z, int64_t ldz, double* __restrict__ Xr, int64_t ldr,
                                                                double* __restrict__ logdet, const double* __restrict__ sigma,
                                                                double* __restrict__ sumsq, const double* __restrict__ tab_x, int T, double y0,
                                                                double ystep, double ylast, const double* __restrict__ tmin,
                                                                const double* __restrict__ tmax, const int* __restrict__ bkt, int nb, int tab_slot,
                                                                int ntiles, int tab0, int ntab) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), GP = cls_gp(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_FEW_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT, FD = TTM_P_FEW_D, HDR = BAND_RT_HDR;
    extern __shared__ __align__(16) double g_lds[];
    const int tid = threadIdx.x;
    const int nc = k1 - k0;
    const int Weven = (T + 4 + 1) & ~1;
    double* itabs = g_lds;                                    // the inverse's tables
    double* ietab = itabs + (size_t)nc * tab_slot;            // {E_i, y_i}
    double* etab = ietab + 2 * Weven;                         // the forward map's exp table
    double* tabs = etab + BAND_ET_DOUBLES;                    // the forward map's splines
    const lds_p etab1 = band_lds(ietab) - 16;
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int N32 = (unsigned int)N;
    const int64_t ldxb = ldx * 8, ldzb = ldz * 8, ldrb = ldr * 8;
    const int nb1 = nb - 1;
    // everything a workgroup stages, requested now
    const D2 ev = *(const D2*)(g_band_etab + 2 * min(tid, TTM_BAND_ET_N - 1));
    D2 sv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) sv[r] = *(const D2*)(U_ + tab0 + min(2 * tid + r * 2 * CT, ntab - 2));
    double tv[FD];
    {
        const double* src = tab_x + min(tid, T - 1);
#pragma unroll
        for (int u = 0; u < FD; ++u) tv[u] = src[(int64_t)min(u, nc - 1) * T];
    }
    const int bc = min(tid >> 8, nc - 1), bw = tid & 255;
    const int4 bv = *(const int4*)(bkt + (int64_t)bc * (nb + 1) + 4 * bw);
    __builtin_amdgcn_sched_barrier(0);
    auto interp = [&](double y_lo, double y_hi, double x_lo, double x_hi, double e_lo, double tgt, double& rr, double& ee) {
        // (the abscissae are np.linspace's to the bit: include/ttm.h)
        const double delta = band_interval_slope(x_lo, x_hi, y_lo, y_hi) * (tgt - x_lo);
        rr = delta + y_lo;
        const double w = (delta * -0.25) * (y_lo + rr);
        double p = fma(kt[0], w, kt[1]);
        p = fma(p, w, kt[2]);
        p = fma(p, w, kt[3]);
        p = fma(p, w, kt[4]);
        p = fma(p, w, kt[5]);
        p = fma(p, w, 1.0);
        p = fma(p, w, 1.0);
        ee = e_lo * p;
    };
    double luni = 0.0;
    bool staged = false;
    auto request = [&](int tile, D2 (&xf)[LAGE][NP], D2 (&xin)[FD][NP]) {
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAGE; ++i) {
                const int cc = kcol0 - LAGE + i;
                const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) xf[i][q] = band_load2(col + roff[q]);
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            const char* col = (const char*)X + (int64_t)(kcol0 + min(j, nc - 1)) * ldxb;
#pragma unroll
            for (int q = 0; q < NP; ++q) xin[j][q] = band_load2(col + roff[q]);
        }
    };
    D2 xf[LAGE][NP], xin[FD][NP];
    if ((int)blockIdx.x < ntiles) request(blockIdx.x, xf, xin);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned int tbase = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        __builtin_amdgcn_sched_barrier(0);
        if (!staged) {
            if (tid < TTM_BAND_ET_N) *(D2*)(etab + 2 * tid) = ev;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = 2 * tid + r * 2 * CT;
                if (i < ntab) *(D2*)(tabs + i) = sv[r];
            }
            if (DENS && sigma) {
                for (int k = 0; k < nc; ++k) luni -= band_log(sigma[k]);
            }
            if (tid < T) {
                ietab[2 * tid] = band_expq_series(tid == T - 1 ? ylast : (double)tid * ystep + y0);
                ietab[2 * tid + 1] = tid == T - 1 ? ylast : (double)tid * ystep + y0;
            }
            if (tid < nc) {
                double* slot = itabs + (size_t)tid * tab_slot;
                double scale, bias;
                band_bucket_params(tmin[tid], tmax[tid], nb, scale, bias);
                slot[0] = scale; slot[1] = bias;
                ((int*)slot)[4] = 0; ((int*)slot)[5] = 0;
                slot[3] = 0.0; slot[4] = 0.0; slot[5] = 0.0;
            }
            if (tid < Weven) {
#pragma unroll
                for (int u = 0; u < FD; ++u) itabs[(size_t)min(u, nc - 1) * tab_slot + HDR + tid] = tid < T ? tv[u] : INFINITY;
            }
            {
                unsigned short* bs = (unsigned short*)(itabs + (size_t)bc * tab_slot + HDR + Weven) + 4 * bw;
                const uint2 pk = {(unsigned int)(bv.x & 0xffff) | ((unsigned int)bv.y << 16), (unsigned int)(bv.z & 0xffff) | ((unsigned int)bv.w << 16)};
                *(uint2*)bs = pk;
            }
            __syncthreads();
            if ((tid >> 8) < nc) {
                const unsigned short* bs = (const unsigned short*)(itabs + (size_t)bc * tab_slot + HDR + Weven);
                const int b4 = bw < 255 ? (int)bs[4 * bw + 4] : bv.w;
                int per = max(bv.y - bv.x, max(bv.z - bv.y, bv.w - bv.z));
                per = max(per, b4 - bv.w);
                for (int o = 32; o > 0; o >>= 1) per = max(per, __shfl_xor(per, o));
                if ((tid & 63) == 0) atomicMax((int*)(itabs + (size_t)bc * tab_slot) + 4, per);
            }
            __syncthreads();
            staged = true;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- forward sweep (k_band_few) ----
        double zk[FD][NS];
        {
            double pend[NS][LAGE];
#pragma unroll
            for (int l = 0; l < LAGE; ++l) {
                const double s0 = P[(int64_t)(k0 + l) * PS];
#pragma unroll
                for (int e = 0; e < NS; ++e) pend[e][l] = s0;
            }
            if (kcol0 > 0) {
#pragma unroll
                for (int i = 0; i < LAGE; ++i) {
                    const bool there = kcol0 - LAGE + i >= 0;
                    cdbl_p rec = P + (int64_t)(k0 + LAG - LAGE + i) * PS;
                    const double start = P[(int64_t)(k0 + i) * PS];
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const double xa = there ? xf[i][q].x : 0.0, xb = there ? xf[i][q].y : 0.0;
                        band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xa, band_expq(etab, xa, kt), pend[2 * q]);
                        band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xb, band_expq(etab, xb, kt), pend[2 * q + 1]);
                    }
                }
            }
            double ss[NS], prod[NS], dmin[NS];
            int pexp[NS];
#pragma unroll
            for (int e = 0; e < NS; ++e) { ss[e] = 0.0; prod[e] = 1.0; dmin[e] = 0.0; pexp[e] = 0; }
#pragma unroll
            for (int j = 0; j < FD; ++j) {
                if (DENS && j == 2 && nc > 2) {
#pragma unroll
                    for (int e = 0; e < NS; ++e) { int ex; prod[e] = frexp(prod[e], &ex); pexp[e] = ex; }
                }
                if (j < nc) {
                    cdbl_p rec = P + (int64_t)(k0 + j + LAG) * PS;
                    const double start = P[(int64_t)(k0 + j + LAGE) * PS];
                    const double sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4], own1 = rec[7];
                    cint_p ri = (cint_p)rec;
                    const int nI = ri[10];
                    const double* tab = tabs + (ri[11] - tab0);
                    char* zcol = (char*)Z + (int64_t)j * ldzb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        double zv[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int e = 2 * q + h;
                            const double x = h ? xin[j][q].y : xin[j][q].x;
                            double m = 0.0, dm = 0.0;
                            if (nI > 0) {
                                if (DENS) band_spline_d(tab, nI, sp_a, sp_b, sp_ds, x, m, dm);
                                else m = band_spline(tab, nI, sp_a, sp_b, sp_ds, x);
                            }
                            const double E = band_expq(etab, x, kt);
                            zv[h] = fma(own1, x, pend[e][0] + m);
                            zk[j][e] = zv[h];
                            if (DENS) {
                                const double dx = fma(dm, sp_ds, own1);
                                ss[e] = fma(zv[h], zv[h], ss[e]);
                                prod[e] *= dx;
                                dmin[e] = fmin(dmin[e], dx);
                            }
                            band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, x, E, pend[e]);
                        }
                        if (Z) {
                            const unsigned int n = tbase + (unsigned int)(q * HALF);
                            char* zp = zcol + (size_t)(n * 8u);
                            if (n + 1 < N32) band_store2<true>(zp, zv[0], zv[1]);
                            else if (n < N32) *(double*)zp = zv[0];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (DENS) {
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const unsigned int n = tbase + (unsigned int)(q * HALF);
                    if (logdet) {
                        const double la = dmin[2 * q] < 0.0 ? NAN : fma((double)pexp[2 * q], 6.93147180559945286e-01, band_log(prod[2 * q])) + luni;
                        const double lb = dmin[2 * q + 1] < 0.0 ? NAN : fma((double)pexp[2 * q + 1], 6.93147180559945286e-01, band_log(prod[2 * q + 1])) + luni;
                        if (n + 1 < N32) band_store2<false>((char*)(logdet + n), la, lb);
                        else if (n < N32) logdet[n] = la;
                    }
                    if (sumsq) {
                        if (n + 1 < N32) band_store2<false>((char*)(sumsq + n), ss[2 * q], ss[2 * q + 1]);
                        else if (n < N32) sumsq[n] = ss[2 * q];
                    }
                }
            }
        }
        // the columns of the workgroup's next tile travel while this tile is inverted (the conditioning columns of THIS tile are
        // still needed: the next tile's go to a second set)
        const bool more = tile + (int)gridDim.x < ntiles;
        D2 xfc[LAGE][NP];
#pragma unroll
        for (int i = 0; i < LAGE; ++i)
#pragma unroll
            for (int q = 0; q < NP; ++q) xfc[i][q] = xf[i][q];
        if (more && !DENS) request(tile + gridDim.x, xf, xin);       // (the density variant has no registers to spare: after the sweep)
        __builtin_amdgcn_sched_barrier(0);
        // ---- inverse sweep (k_band_few_inverse), targets from registers ----
        {
            double pend[NS][LAGE];
#pragma unroll
            for (int l = 0; l < LAGE; ++l) {
                const double s0 = P[(int64_t)(k0 + l) * PS + 1];
#pragma unroll
                for (int e = 0; e < NS; ++e) pend[e][l] = s0;
            }
            if (kcol0 > 0) {
#pragma unroll
                for (int i = 0; i < LAGE; ++i) {
                    const bool there = kcol0 - LAGE + i >= 0;
                    cdbl_p rec = P + (int64_t)(k0 + LAG - LAGE + i) * PS;
                    const double start = P[(int64_t)(k0 + i) * PS + 1];
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const double xa = there ? xfc[i][q].x : 0.0, xb = there ? xfc[i][q].y : 0.0;
                        band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xa, there ? band_expq_series(xa) : 1.0, pend[2 * q]);
                        band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, xb, there ? band_expq_series(xb) : 1.0, pend[2 * q + 1]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < FD; ++j) {
                if (j < nc) {
                    cdbl_p rec = P + (int64_t)(k0 + j + LAG) * PS;
                    const double start = P[(int64_t)(k0 + j + LAGE) * PS + 1];
                    const double* slot = itabs + (size_t)j * tab_slot;
                    const double scale = slot[0], bias = slot[1];
                    const int per = __builtin_amdgcn_readfirstlane(((const int*)slot)[4]);
                    const int pm = max(per, 1);
                    const bool deg = pm + 3 >= T || per > 255;
                    const lds_p xsl = band_lds(slot + HDR);
                    const lds_p bkl = band_lds(slot + HDR + Weven);
                    const double wl = band_lds_f64(xsl + 8 * (deg ? 1 : pm)), wh = band_lds_f64(xsl + 8 * (deg ? 1 : T - 2));
                    const int nph = per <= 3 ? 1 : per <= 15 ? 2 : per <= 63 ? 3 : 4;
                    double traw[NS], tg[NS], r[NS], E[NS];
                    unsigned long long outl = deg ? ~0ull : 0ull;
                    int pos[NS];
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        const double z = zk[j][e];
                        traw[e] = z - pend[e][0];
                        tg[e] = fmin(fmax(traw[e], wl), wh);
                        outl |= __builtin_amdgcn_ballot_w64(traw[e] != tg[e]);
                        const int bi = min((int)fma(tg[e], scale, bias), nb1);
                        pos[e] = (int)*(const __attribute__((address_space(3))) unsigned short*)(bkl + 2 * bi);
                    }
                    for (int ph = 0, s = 1 << (2 * (nph - 1)); ph < nph; ++ph, s >>= 2) {
                        double qv[NS][3];
#pragma unroll
                        for (int e = 0; e < NS; ++e)
#pragma unroll
                            for (int i = 0; i < 3; ++i) qv[e][i] = band_lds_f64_single(xsl + 8 * min(pos[e] + (i + 1) * s - 1, T + 3));
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            int c = 0;
#pragma unroll
                            for (int i = 0; i < 3; ++i) c += qv[e][i] < tg[e] ? 1 : 0;
                            pos[e] += c * s;
                        }
                    }
                    {
                        D2 ey[NS];
                        double xlo[NS], xhi[NS], yhi[NS];
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            const int ps1 = band_med3(pos[e], 1, T - 1);
                            ey[e] = band_lds_pair(etab1 + 16 * ps1);
                            yhi[e] = band_lds_f64_single(etab1 + 16 * ps1 + 24);
                            const lds_p xp = xsl + 8 * ps1;
                            xlo[e] = band_lds_f64(xp - 8);
                            xhi[e] = band_lds_f64_single(xp);
                        }
#pragma unroll
                        for (int e = 0; e < NS; ++e) interp(ey[e].y, yhi[e], xlo[e], xhi[e], ey[e].x, tg[e], r[e], E[e]);
                    }
                    if (outl != 0) {
                        const double* xg = tab_x + (int64_t)j * T;
                        const double lo = tmin[j], hi = tmax[j];
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            if (deg || traw[e] != tg[e]) {
                                double t = traw[e];
                                const double cl = fmin(fmax(t, lo), hi);
                                t = t != t ? t : cl;
                                int a = 0, b = T;
                                while (a < b) {
                                    const int mid = (a + b) >> 1;
                                    if (xg[mid] < t) a = mid + 1; else b = mid;
                                }
                                const int i = min(max(a, 1), T - 1);
                                interp((double)(i - 1) * ystep + y0, i == T - 1 ? ylast : (double)i * ystep + y0, xg[i - 1], xg[i], band_expq_series((double)(i - 1) * ystep + y0), t, r[e], E[e]);
                            }
                        }
                    }
#pragma unroll
                    for (int e = 0; e < NS; ++e) band_push_e<DB, DA, GP, LAGE, PLAIN>(rec + TTM_P_HDR, start, r[e], E[e], pend[e]);
                    char* xcol = (char*)Xr + (int64_t)(kcol0 + j) * ldrb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const unsigned int n = tbase + (unsigned int)(q * HALF);
                        char* xp = xcol + (size_t)(n * 8u);
                        if (n + 1 < N32) band_store2<true>(xp, r[2 * q], r[2 * q + 1]);
                        else if (n < N32) *(double*)xp = r[2 * q];
                    }
                }
            }
        }
        if (more && DENS) request(tile + gridDim.x, xf, xin);
    }
}

// ---------------------------------------------------------------------------
// root searches in push form: S_c(x) = z_c with S_c(x) = pend[0] + own1 x + G_c(x), G_c the component's resident spline - no
// inverse tables, no images.  One routine, band_search_rows, on the rows of a thread at once.  Both methods open alike:
// bracket [-2, 2], its ends swapped where flo > fhi, shifted by twice its width while both values lie on one side of zero (at
// most 2000 shifts; flo = 0 or a NaN ends them).  BIS then selects the tail:
//  - safeguarded Newton (root_finder = 'newton', ttm_inverse_newton): the iteration is sample_newton's (csrc/ttm_eval.h),
//    statement for statement: secant start, Newton step with dS/dx, midpoint whenever the step leaves the bracket (a zero
//    derivative sends it to infinity: midpoint), stop at |S - z| <= 1e-9 or 100 trial points; a row without a sign change (NaN
//    target, a component that is not monotone) ends at the last bracket point tried.
//  - the reference's bisection (root_finder = 'reference', ttm_inverse_bisect without a cap): sample_bisect (csrc/ttm_eval.h)
//    statement for statement: midpoints only - lo = mid where fm < 0, hi = mid where fm > 0, stop at !(|fm| > 1e-9) or after
//    100 midpoints.  There is no exit for a bracket without a sign change (sample_newton has one): whatever bracket the shifts
//    end with is bisected, and a NaN target stops at the first midpoint, 0.  No derivative, no division: the loop's state is
//    lo, hi, t and r per row.
// A finished row keeps its result and rides along (selects, no branches), so the dependent chains of the rows overlap; the
// loops end when every lane is done.  The residual is taken against t = z - pend[0], the target of the monotone part (what
// band_inverse_tile looks up): one running value per row instead of two through the loops.
// ---------------------------------------------------------------------------
// a / b: reciprocal + two Newton steps + one correction of the quotient (b = 0, infinite or NaN: not a finite quotient)
__device__ __forceinline__ double band_div(double a, double b) {
    double rc = __builtin_amdgcn_rcp(b);
    rc = fma(fma(-b, rc, 1.0), rc, rc);
    rc = fma(fma(-b, rc, 1.0), rc, rc);
    const double q = a * rc;
    return fma(fma(-b, q, a), rc, q);
}

// exp(-x^2/4) of a solved column: band_expq, and exactly 0 where the true value has underflowed - a search that ran away
// (a target no x reaches: |x| ~ 1e307, or infinite) then pushes 0 x inf = NaN on, as the term-table evaluator does, and
// not the table's last entry times infinity
__device__ __forceinline__ double band_expq_far(const double* etab, double x, cdbl_p kt) {
    const double E = band_expq(etab, x, kt);
    return fabs(x) > 60.0 ? 0.0 : E;
}

// sp(der, x, g, dg): the spline and (der) its derivative with respect to the local coordinate; sp_ds: d local / dx (the
// bisection ignores it).  t: the rows' targets of the monotone part, r: the last trial points (BIS: the last midpoints); live:
// the row is one of the caller's own (a row that is not searches nothing and counts nothing: r = +2).  Returns the most trial
// points (BIS: midpoints) a live row needed.
// (The bracket stays in this function: as a routine of its own, its four arrays by reference, it changes the register
// allocation of the Newton kernels - OPTLOG rounds 11 and 13.)
template <int NS, bool OWN, bool BIS, class SP>
__device__ __forceinline__ int band_search_rows(const SP& sp, double own1, double sp_ds, const double (&t)[NS], const bool (&live)[NS],
                                                double (&r)[NS]) {
    auto value = [&](double x, double g) { return OWN ? fma(own1, x, g) : g; };
    double lo[NS], hi[NS], flo[NS], fhi[NS];
    bool widen = false;
    {
        double gl, gh, d;
        sp(std::false_type(), -2.0, gl, d);                   // (the first two trial points are the same for every row)
        sp(std::false_type(), 2.0, gh, d);
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            const double a = value(-2.0, gl) - t[e], b = value(2.0, gh) - t[e];
            const bool sw = a > b;
            flo[e] = sw ? b : a; fhi[e] = sw ? a : b;
            lo[e] = sw ? 2.0 : -2.0; hi[e] = sw ? -2.0 : 2.0;
            r[e] = 2.0;
            widen = widen || (live[e] && flo[e] * fhi[e] > 0.0);
        }
    }
    for (int guard = 0; guard < 2000 && widen; ++guard) {
        widen = false;
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            const bool need = live[e] && flo[e] * fhi[e] > 0.0;
            const bool sw = flo[e] > fhi[e];
            const double l = sw ? hi[e] : lo[e], h = sw ? lo[e] : hi[e], fl = sw ? fhi[e] : flo[e], fh = sw ? flo[e] : fhi[e];
            const double diff = h - l;
            const bool down = fl > 0.0;                       // (need: both values on one side of zero)
            double xt = down ? l - diff * 2.0 : h + diff * 2.0;
            xt = need ? xt : r[e];
            double g, d;
            sp(std::false_type(), xt, g, d);
            const double ft = value(xt, g) - t[e];
            if (need) {
                lo[e] = down ? xt : h; flo[e] = down ? ft : fh;
                hi[e] = down ? l : xt; fhi[e] = down ? fl : ft;
                r[e] = xt;
            }
            widen = widen || (need && flo[e] * fhi[e] > 0.0);
            if (e & 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (BIS) {
        bool act[NS], any = false;
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            act[e] = live[e];
            any = any || act[e];
        }
        int n = 0;
        while (any && n < 100) {
            ++n;
            any = false;
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                const double mid = (lo[e] + hi[e]) * 0.5;         // (a finished row's bracket stands: the same point again)
                double g, d;
                sp(std::false_type(), mid, g, d);
                const double fm = value(mid, g) - t[e];
                lo[e] = (act[e] && fm < 0.0) ? mid : lo[e];
                hi[e] = (act[e] && fm > 0.0) ? mid : hi[e];
                r[e] = act[e] ? mid : r[e];
                act[e] = act[e] && fabs(fm) > 1e-9;
                any = any || act[e];
                if (e & 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        return n;
    } else {
        // (from here on r is the trial point itself: a finished row's stays, a row stopped by the cap keeps the last one evaluated)
        bool act[NS], any = false;
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            act[e] = live[e] && flo[e] * fhi[e] <= 0.0;           // (false: NaN, or no sign change within the shifts)
            const double mid = (lo[e] + hi[e]) * 0.5;
            double xs = lo[e] - flo[e] * band_div(hi[e] - lo[e], fhi[e] - flo[e]);      // secant start
            xs = fhi[e] != flo[e] ? xs : mid;
            xs = (xs > fmin(lo[e], hi[e]) && xs < fmax(lo[e], hi[e])) ? xs : mid;
            r[e] = act[e] ? xs : r[e];
            any = any || act[e];
        }
        int n = 0;
        while (any && n < 100) {
            ++n;
            any = false;
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                double g, dg;
                sp(std::true_type(), r[e], g, dg);
                const double f = value(r[e], g) - t[e];
                const double ds = OWN ? fma(dg, sp_ds, own1) : dg * sp_ds;
                const bool go = act[e] && fabs(f) > 1e-9;
                const double l = f < 0.0 ? r[e] : lo[e], h = f < 0.0 ? hi[e] : r[e];
                double xn = r[e] - band_div(f, ds);
                xn = (xn > fmin(l, h) && xn < fmax(l, h)) ? xn : (l + h) * 0.5;
                lo[e] = go ? l : lo[e]; hi[e] = go ? h : hi[e];
                r[e] = (go && n < 100) ? xn : r[e];
                act[e] = go;
                any = any || go;
                if (e & 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        return n;
    }
}

// the most trial points of the wave's rows into iters[c] (one vector atomic per wave and column; 0: nothing to record)
__device__ __forceinline__ void band_iters_max(int* iters, int c, int it) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) it = max(it, __shfl_down(it, off, 64));
    if ((threadIdx.x & 63) == 0 && it > 0) atomicMax(iters + c, it);
}

// Maps of more than TTM_P_FEW_D components (C5): the structure of k_band_forward - one workgroup per CU and row chunk, the
// block's splines and the exp table resident, four rows per thread as two 16-byte pairs, column c + 1 of Z requested at the
// top of step c, x_c stored at the end of its step.  With several blocks a tile re-reads the LAG columns in front of a block
// (its own stores, or conditioning columns) and pushes them again with the same arithmetic: a row's result does not depend on
// the chunking.  A pair whose second row does not exist (odd N) carries its first row twice: padding never enters a search.
// LDS: [E table: 2 x 801 | splines of the block's components, as they stand in the U section]
// BIS: the search of a step is the reference's bisection (reported as k_band_bisect; iters: midpoints), else the Newton search
// (reported as k_band_newton; iters: trial points) - the only place the two instantiations differ.
template <int CLS, int LAG, bool OWN, bool BIS>
__global__ __launch_bounds__(BAND_CT) void k_band_search(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                         const double* __restrict__ Z, int64_t ldz, double* X, int64_t ldx, int64_t N,
                                                         int* __restrict__ iters, int64_t rows_per_wg, int Bc) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT;
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    band_stage<false>(etab, g_band_etab, 2 * TTM_BAND_ET_N);      // (waited for with the first block's splines)
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int c1_32 = (unsigned int)c1, N32 = (unsigned int)N;
    const int64_t ldzb = ldz * 8, ldxb = ldx * 8;

    for (int kb = k0; kb < k1; kb += Bc) {
        const int ke = kb + Bc < k1 ? kb + Bc : k1;
        __syncthreads();                                      // every wave is done with the previous block's splines
        int tab0;
        {
            cint_p rb = (cint_p)(P + (int64_t)(kb + LAG) * PS), re = (cint_p)(P + (int64_t)(ke - 1 + LAG) * PS);
            tab0 = rb[11];
            const int n = re[11] + TTM_U_TSTRIDE * re[10] - tab0;           // doubles (even)
            band_stage(tabs, U_ + tab0, n);
        }
        __syncthreads();
        const int colb = kcol0 + (kb - k0);                   // column of component kb
        for (int tile = 0; tile < ntile; ++tile) {
            const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
            const bool full = c0 + (int64_t)(tile + 1) * ROWS <= c1;
            unsigned int roff[NP];
            bool single[NP];                                  // the pair's second row is padding
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                unsigned int n = tbase + (unsigned int)(q * HALF);
                n = n < last_pair ? n : last_pair;
                roff[q] = n * 8u;
                single[q] = n + 1 >= N32;
            }
            auto load = [&](const char* col, int q) {
                D2 v = band_load2(col + roff[q]);
                v.y = single[q] ? v.x : v.y;
                return v;
            };
            double pend[NS][LAG];
#pragma unroll
            for (int l = 0; l < LAG; ++l) {
                const double s = P[(int64_t)(kb + l) * PS];
#pragma unroll
                for (int e = 0; e < NS; ++e) pend[e][l] = s;
            }
            if (colb > 0) {
                // the LAG columns in front of the block, pushed without being solved (a column that does not exist has an
                // all-zero record: with x = 0, E = 1 its step only shifts the sums)
                for (int i = 0; i < LAG; ++i) {
                    const int cc = colb - LAG + i;
                    cdbl_p rec = P + (int64_t)(kb + i) * PS;
                    const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        D2 xv = load(col, q);
                        if (cc < 0) { xv.x = 0.0; xv.y = 0.0; }
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.x, band_expq_far(etab, xv.x, kt), pend[2 * q]);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.y, band_expq_far(etab, xv.y, kt), pend[2 * q + 1]);
                    }
                }
            }
            const char* zcol = (const char*)Z + (int64_t)(kb - k0) * ldzb;
            char* xcol = (char*)X + (int64_t)colb * ldxb;
            cdbl_p rec = P + (int64_t)(kb + LAG) * PS;
            D2 za[NP], zb[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) za[q] = load(zcol, q);
            auto step = [&](int j, const D2 (&zc)[NP], D2 (&zn)[NP]) {
                {
                    const char* znext = j + 1 < ke ? zcol + ldzb : zcol;      // (past the block: a harmless re-read)
#pragma unroll
                    for (int q = 0; q < NP; ++q) zn[q] = load(znext, q);
                }
                __builtin_amdgcn_sched_barrier(0);
                const double start = rec[0], sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4];
                const double own1 = OWN ? rec[7] : 0.0;
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];                        // (OWN: 0 - no special terms, no spline: the component is linear)
                const double* tab = tabs + (ri[11] - tab0);
                auto sp = [&](auto der, double x, double& g, double& dg) {
                    if (OWN && nI <= 0) { g = 0.0; dg = 0.0; }
                    else if (decltype(der)::value) band_spline_d(tab, nI, sp_a, sp_b, sp_ds, x, g, dg);
                    else { g = band_spline(tab, nI, sp_a, sp_b, sp_ds, x); dg = 0.0; }
                };
                // (rows of the tile beyond the chunk belong to the next workgroup: not searched, not counted, not stored)
                double tg[NS], r[NS];
                bool live[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    tg[e] = ((e & 1) ? zc[e >> 1].y : zc[e >> 1].x) - pend[e][0];
                    live[e] = full || tbase + (unsigned int)((e >> 1) * HALF + (e & 1)) < c1_32;
                }
                const int it = band_search_rows<NS, OWN, BIS>(sp, own1, sp_ds, tg, live, r);
                // x_c is pushed on to the components that read it, and stored
#pragma unroll
                for (int e = 0; e < NS; ++e) band_push<DB, DA, LAG>(rec + TTM_P_HDR, start, r[e], band_expq_far(etab, r[e], kt), pend[e]);
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const unsigned int n = tbase + (unsigned int)(q * HALF);
                    char* xp = xcol + (size_t)(n * 8u);
                    if (full || n + 1 < c1_32) band_store2<false>(xp, r[2 * q], r[2 * q + 1]);
                    else if (n < c1_32) *(double*)xp = r[2 * q];
                }
                band_iters_max(iters, j - k0, it);
                rec += PS; zcol += ldzb; xcol += ldxb;
            };
            int j = kb;
            for (; j + 1 < ke; j += 2) {
                step(j, za, zb);
                step(j + 1, zb, za);
            }
            if (j < ke) step(j, za, zb);
        }
    }
}

// Maps of a few components (C2b, C3, EX03, the filter and block maps): tiles, staging and conditioning-column prologue of
// k_band_few / k_band_few_inverse - the exp table, every spline and all columns of the tile requested together - without
// any table; monotone part own1 x + G_c(x) (a component without a spline is linear: the first Newton step is exact).  One
// shape per order class and record lag: groups beyond a sweep's reach are zeros in the records.
// BIS: the reference's bisection (reported as k_band_few_bisect; a component without a spline is bisected like any other),
// else the Newton search (reported as k_band_few_newton) - the only place the two instantiations differ.
template <int CLS, int LAG, bool BIS>
__global__ __launch_bounds__(BAND_CT) void k_band_few_search(const double* __restrict__ U_, int64_t p_off, int k0, int k1, int kcol0,
                                                             const double* __restrict__ Z, int64_t ldz, double* X, int64_t ldx, int64_t N,
                                                             int* __restrict__ iters, int ntiles, int tab0, int ntab) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), GP = cls_gp(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_FEW_NS, NP = NS / 2, CT = BAND_CT, ROWS = NS * CT, HALF = 2 * CT, FD = TTM_P_FEW_D;
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int nc = k1 - k0;
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int N32 = (unsigned int)N;
    const int64_t ldzb = ldz * 8, ldxb = ldx * 8;
    // the exp table and the splines: requested now, written to LDS after the first tile's columns have been requested
    const D2 ev = *(const D2*)(g_band_etab + 2 * min(tid, TTM_BAND_ET_N - 1));
    D2 sv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) sv[r] = *(const D2*)(U_ + tab0 + min(2 * tid + r * 2 * CT, ntab - 2));
    __builtin_amdgcn_sched_barrier(0);
    // every column of a tile: the conditioning columns in front of the first component (already in X) and z; a pair whose
    // second row is padding carries its first row twice
    auto request = [&](int tile, D2 (&xf)[LAG][NP], D2 (&zin)[FD][NP]) {
        unsigned int roff[NP];
        bool single[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
            single[q] = n + 1 >= N32;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAG; ++i) {
                const int cc = kcol0 - LAG + i;
                const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) { xf[i][q] = band_load2(col + roff[q]); xf[i][q].y = single[q] ? xf[i][q].x : xf[i][q].y; }
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            const char* col = (const char*)Z + (int64_t)min(j, nc - 1) * ldzb;
#pragma unroll
            for (int q = 0; q < NP; ++q) { zin[j][q] = band_load2(col + roff[q]); zin[j][q].y = single[q] ? zin[j][q].x : zin[j][q].y; }
        }
    };
    D2 xf[LAG][NP], zin[FD][NP];
    if ((int)blockIdx.x < ntiles) request(blockIdx.x, xf, zin);
    bool staged = false;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned int tbase = (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        __builtin_amdgcn_sched_barrier(0);
        if (!staged) {
            if (tid < TTM_BAND_ET_N) *(D2*)(etab + 2 * tid) = ev;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = 2 * tid + r * 2 * CT;
                if (i < ntab) *(D2*)(tabs + i) = sv[r];
            }
            __syncthreads();
            staged = true;
        }
        double pend[NS][LAG];
#pragma unroll
        for (int l = 0; l < LAG; ++l) {
            const double s0 = P[(int64_t)(k0 + l) * PS];
#pragma unroll
            for (int e = 0; e < NS; ++e) pend[e][l] = s0;
        }
        if (kcol0 > 0) {
#pragma unroll
            for (int i = 0; i < LAG; ++i) {
                // (record of the column LAG - i in front of component k0; the chain it starts is component k0 + i's)
                const bool there = kcol0 - LAG + i >= 0;
                cdbl_p rec = P + (int64_t)(k0 + i) * PS;
                const double start = rec[0];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const double xa = there ? xf[i][q].x : 0.0, xb = there ? xf[i][q].y : 0.0;
                    band_push_e<DB, DA, GP, LAG, true>(rec + TTM_P_HDR, start, xa, band_expq_far(etab, xa, kt), pend[2 * q]);
                    band_push_e<DB, DA, GP, LAG, true>(rec + TTM_P_HDR, start, xb, band_expq_far(etab, xb, kt), pend[2 * q + 1]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FD; ++j) {
            if (j < nc) {
                cdbl_p rec = P + (int64_t)(k0 + j + LAG) * PS;
                const double start = rec[0];                  // (of the component LAG columns on)
                const double sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4], own1 = rec[7];
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];                        // (0: no special terms, no spline)
                const double* tab = tabs + (ri[11] - tab0);
                auto sp = [&](auto der, double x, double& g, double& dg) {
                    g = 0.0; dg = 0.0;
                    if (nI > 0) {
                        if (decltype(der)::value) band_spline_d(tab, nI, sp_a, sp_b, sp_ds, x, g, dg);
                        else g = band_spline(tab, nI, sp_a, sp_b, sp_ds, x);
                    }
                };
                double tg[NS], r[NS];
                bool live[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    tg[e] = ((e & 1) ? zin[j][e >> 1].y : zin[j][e >> 1].x) - pend[e][0];
                    live[e] = tbase + (unsigned int)e < N32;
                }
                const int it = band_search_rows<NS, true, BIS>(sp, own1, sp_ds, tg, live, r);
#pragma unroll
                for (int e = 0; e < NS; ++e) band_push_e<DB, DA, GP, LAG, true>(rec + TTM_P_HDR, start, r[e], band_expq_far(etab, r[e], kt), pend[e]);
                char* xcol = (char*)X + (int64_t)(kcol0 + j) * ldxb;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const unsigned int n = tbase + (unsigned int)(q * HALF);
                    char* xp = xcol + (size_t)(n * 8u);
                    if (n + 1 < N32) band_store2<true>(xp, r[2 * q], r[2 * q + 1]);
                    else if (n < N32) *(double*)xp = r[2 * q];
                }
                band_iters_max(iters, j, it);
            }
        }
        // (the searches are bound by their arithmetic, and their state leaves no registers for a second set of columns: the
        // workgroup's next tile is requested after this one)
        if (tile + (int)gridDim.x < ntiles) request(tile + gridDim.x, xf, zin);
    }
}

// ---------------------------------------------------------------------------
// score of the pullback density in push form (csrc/ttm_score.h, include/ttm.h: ttm_score):
//
//     G_j = -g_j sum_{l = 0..LAG} S_{j+l}(u) dS_{j+l}/du_c (u) + m_j''(t) / m_j'(t),      c the column of component j.
//
// One sweep over the columns, the structure of k_band_density.  At column c a row forms S_c = pend[0] + own1 x + m(x) and pushes
// x on exactly as band_push does; the same loop over the record's groups also gives f'_{c+l, c}(x), l = 1..LAG, which wait in
// registers (dq) until S_{c+l} is known.  S_c then closes one term of each of the LAG + 1 open score columns c - LAG .. c:
// column c - LAG is complete and stored at step c, the last LAG columns are flushed behind the sweep.  Live per row:
// pend[LAG], acc[LAG + 1], LAG (LAG + 1) / 2 derivatives.
//   * the spline is gathered once for m, m', m'' (band_spline_d2: three recurrences over the six aligned 16-byte reads); with
//     ld_affine the log-determinant term is taken at t = scale x + shift: a second gather for m'(t), m''(t) behind a uniform
//     branch - the standardised call pays for one;
//   * B and B' in one fused Horner pass, A' likewise next to band_push's own chain for A (band_group_d): the pushed values are
//     band_push's, bit for bit; the groups of a record are taken one after the other for all rows, so that one group's
//     coefficients occupy scalar registers at a time;
//   * a non-finite sample makes every score of the row that depends on it NaN (x 0 on the constant slope of a linear own term);
//     beyond a spline's support the tail column is exactly linear: m'' = 0.
// Conditioning columns in front of the first component are pushed first and get no output.  With several blocks of resident
// splines a tile walks the blocks in turn (the row state stays in registers; a single block - C5 - is staged once per launch).
// The pair table is requested by DMA at the top and is complete behind the first stage's wait and barrier: nothing reads it before.
// Two rows per thread for every LAG (at LAG = 2 the step is bound by its arithmetic - about twice k_band_forward's FMAs per
// column - not by the column stream); workgroups of 1024 threads for C5's shape, of 512 for the others (band_score_ct).
// LDS: [E table: 2 x 801 | splines of the block's components, as they stand in the U section]
// ---------------------------------------------------------------------------
// value (VAL), first derivative and HALF the second derivative of the spline with respect to the local coordinate
template <bool VAL>
__device__ __forceinline__ void band_spline_d2(const double* tab, int nI, double sp_a, double sp_b, double sp_ds, double x, double& m, double& dm,
                                               double& hd2m) {
    const int col = band_med3((int)fma(x, sp_b, sp_a), 0, nI - 1);
    const double* cp = (const double*)((const char*)tab + __umul24((unsigned int)col, TTM_U_TSTRIDE * 8));
    double c[12];
#pragma unroll
    for (int i = 0; i < 12; i += 2) { const D2 v = *(const D2*)(cp + i); c[i] = v.x; c[i + 1] = v.y; }
    if (!VAL) asm volatile("" :: "v"(c[0]));                  // (keeps the six aligned 16-byte reads, see band_spline_dd)
    const double s = fma(x, sp_ds, cp[12]);
    // (the first two trips of the three recurrences, whose leading terms are zero, written out)
    double a = fma(c[11], s, c[10]), da = c[11], dda = da;
    da = fma(da, s, a);
    a = fma(a, s, c[9]);
#pragma unroll
    for (int i = 8; i >= (VAL ? 0 : 1); --i) {
        dda = fma(dda, s, da);
        da = fma(da, s, a);
        a = fma(a, s, c[i]);
    }
    if (!VAL) {
        dda = fma(dda, s, da);
        da = fma(da, s, a);
    }
    m = a; dm = da; hd2m = dda;
}

// one group of band_push with its derivative: returns base + A(x) - A[0] + E B(x) - the operations of band_push, in its order - and
// d = f'(x) = A'(x) + E (B'(x) - x B(x) / 2), B and B' (A and A') in one fused Horner pass each.  c: B[0..DB], A[1..DA]; hx = -x / 2
template <int DB, int DA, class C>
__device__ __forceinline__ double band_group_d(const C c, double base, double x, double hx, double E, double& d) {
    double b = c[DB], db = b;
    b = fma(b, x, c[DB - 1]);
#pragma unroll
    for (int i = DB - 2; i >= 0; --i) {
        db = fma(db, x, b);
        b = fma(b, x, c[i]);
    }
    double a = c[DB + DA], da = a;
#pragma unroll
    for (int i = DA - 1; i >= 1; --i) {
        if (i != DA - 1) da = fma(da, x, a);
        a = fma(a, x, c[DB + i]);
    }
    if (DA > 1) da = fma(da, x, a);
    a = fma(a, x, base);
    d = fma(E, fma(hx, b, db), da);
    return fma(E, b, a);
}

// n doubles into LDS by a workgroup of CT threads (band_stage: BAND_CT)
template <int CT>
__device__ __forceinline__ void band_stage_ct(double* lds_dst, const double* src, int n) {
    const int units = n >> 1;
    const unsigned int base = band_lds_addr(lds_dst);
    for (int u0 = 0; u0 < units; u0 += CT) {
        const int u = u0 + (int)threadIdx.x;
        if (u < units) band_dma16(src + 2 * (size_t)u, __builtin_amdgcn_readfirstlane(base + (unsigned int)(u0 + ((int)threadIdx.x & ~63)) * 16u));
    }
}

#define BAND_SCORE_NS 2
// threads per workgroup, so that no instantiation spills: BAND_CT (128 registers per thread) holds the step of C5's shape - degree
// class 1, two groups per record; the longer Horner chains of the other classes and the row state of the longer records (LAG = 5:
// 52 registers per row) take half a workgroup (256 registers per thread)
__host__ __device__ constexpr int band_score_ct(int cls, int lag) { return cls == 1 && lag == 2 ? BAND_CT : BAND_CT / 2; }
template <int CLS, int LAG, bool OWN>
__global__ __launch_bounds__(band_score_ct(CLS, LAG)) void k_band_score(const double* __restrict__ U_, int64_t p_off, int D, int kcol0,
                                                        const double* __restrict__ X, int64_t ldx, int64_t N, double* __restrict__ G,
                                                        int64_t ldg, const double* __restrict__ g_scale,
                                                        const double* __restrict__ ld_affine, int64_t rows_per_wg, int Bc) {
    constexpr int DB = cls_db(CLS), DA = cls_da(CLS), PS = rec_stride(CLS, LAG);
    constexpr int NS = BAND_SCORE_NS, NP = NS / 2, CT = band_score_ct(CLS, LAG), ROWS = NS * CT, HALF = 2 * CT, NQ = LAG * (LAG + 1) / 2;
    constexpr int GP = cls_gp(CLS);
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    double* tabs = g_lds + BAND_ET_DOUBLES;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * rows_per_wg;
    if (c0 >= N) return;
    const int64_t c1 = c0 + rows_per_wg < N ? c0 + rows_per_wg : N;
    const int ntile = (int)((c1 - c0 + ROWS - 1) / ROWS);
    band_stage_ct<CT>(etab, g_band_etab, 2 * TTM_BAND_ET_N);      // (waited for with the first block's splines)
    cdbl_p P = (cdbl_p)(U_ + p_off);
    cdbl_p kt = (cdbl_p)g_band_taylor;
    cdbl_p gs = (cdbl_p)g_scale, af = (cdbl_p)ld_affine;
    const unsigned int last_pair = (unsigned int)(((N + 1) & ~(int64_t)1) - 2);
    const unsigned int c1_32 = (unsigned int)c1;
    const int64_t ldxb = ldx * 8, ldgb = ldg * 8;
    int tab0 = 0;
    auto stage = [&](int kb, int ke) {                        // the splines of the components [kb, ke), as k_band_search stages them
        cint_p rb = (cint_p)(P + (int64_t)(kb + LAG) * PS), re = (cint_p)(P + (int64_t)(ke - 1 + LAG) * PS);
        tab0 = rb[11];
        band_stage_ct<CT>(tabs, U_ + tab0, re[11] + TTM_U_TSTRIDE * re[10] - tab0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    const bool one = Bc >= D;                                 // one block: staged once, for every tile
    if (one) {
        stage(0, D);
        __syncthreads();
    }
    for (int tile = 0; tile < ntile; ++tile) {
        const unsigned int tbase = (unsigned int)c0 + (unsigned int)tile * (unsigned int)ROWS + 2u * (unsigned int)tid;
        unsigned int roff[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            unsigned int n = tbase + (unsigned int)(q * HALF);
            n = n < last_pair ? n : last_pair;
            roff[q] = n * 8u;
        }
        // a pair of score values of column jc: rows of the tile beyond the chunk belong to the next workgroup, the second row of
        // the last pair may not exist
        auto store = [&](int jc, int q, double v0, double v1) {
            const unsigned int n = tbase + (unsigned int)(q * HALF);
            char* gp = (char*)G + (int64_t)jc * ldgb + (size_t)(n * 8u);
            if (n + 1 < c1_32) band_store2<false>(gp, v0, v1);
            else if (n < c1_32) *(double*)gp = v0;
        };
        double pend[NS][LAG], acc[NS][LAG + 1], dq[NS][NQ];  // dq[l (l - 1) / 2 + a]: f'_{., l} of a + 1 steps ago, l = 1..LAG
#pragma unroll
        for (int e = 0; e < NS; ++e) {
#pragma unroll
            for (int l = 0; l < LAG; ++l) pend[e][l] = P[(int64_t)l * PS];
#pragma unroll
            for (int l = 0; l <= LAG; ++l) acc[e][l] = 0.0;
#pragma unroll
            for (int i = 0; i < NQ; ++i) dq[e][i] = 0.0;
        }
        for (int kb = 0; kb < D; kb += Bc) {
            const int ke = kb + Bc < D ? kb + Bc : D;
            if (!one) {
                __syncthreads();                              // every wave is done with the previous block's splines
                stage(kb, ke);
                __syncthreads();
            }
            if (kb == 0 && kcol0 > 0) {
                // the LAG columns in front of the first component (conditioning columns; a column that does not exist has an all-zero
                // record: with x = 0, E = 1 its step only shifts the sums): pushed, no output.
                // Behind the first block's barrier: band_expq reads the pair table, which every wave's DMA has to have delivered
                for (int i = 0; i < LAG; ++i) {
                    const int cc = kcol0 - LAG + i;
                    cdbl_p rec = P + (int64_t)i * PS;
                    const char* col = (const char*)X + (int64_t)(cc < 0 ? 0 : cc) * ldxb;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        D2 xv = band_load2(col + roff[q]);
                        if (cc < 0) { xv.x = 0.0; xv.y = 0.0; }
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.x, band_expq(etab, xv.x, kt), pend[2 * q]);
                        band_push<DB, DA, LAG>(rec + TTM_P_HDR, rec[0], xv.y, band_expq(etab, xv.y, kt), pend[2 * q + 1]);
                    }
                }
            }
            const char* xcol = (const char*)X + (int64_t)(kcol0 + kb) * ldxb;
            cdbl_p rec = P + (int64_t)(kb + LAG) * PS;
            D2 xa[NP], xb[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) xa[q] = band_load2(xcol + roff[q]);
            auto step = [&](int j, const D2 (&xc)[NP], D2 (&xn)[NP]) {
                {
                    const char* xnext = j + 1 < ke ? xcol + ldxb : xcol;      // (past the block: a harmless re-read)
#pragma unroll
                    for (int q = 0; q < NP; ++q) xn[q] = band_load2(xnext + roff[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
                const double start = rec[0], sp_a = rec[2], sp_b = rec[3], sp_ds = rec[4];
                const double own1 = OWN ? rec[7] : 0.0;
                const double c2 = 2.0 * (sp_ds * sp_ds);      // m'' = c2 x half the second derivative in the local coordinate
                cint_p ri = (cint_p)rec;
                const int nI = ri[10];                        // (0: no special terms, no spline - the component is linear)
                const double* tab = tabs + (ri[11] - tab0);
                double gl[LAG + 1];                           // factor on the Gaussian part of the columns j - l
#pragma unroll
                for (int l = 0; l <= LAG; ++l) gl[l] = gs ? gs[j - l < 0 ? 0 : j - l] : 1.0;
                const double t_a = af ? af[2 * j] : 1.0, t_b = af ? af[2 * j + 1] : 0.0;
                // row by row: S, which closes one term of every open column (acc[l] is column j - l), and the new column's start
                double xr[NS], Er[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    const double x = (e & 1) ? xc[e >> 1].y : xc[e >> 1].x;
                    double m = 0.0, dm = 0.0, hd2 = 0.0;
                    if (nI > 0) band_spline_d2<true>(tab, nI, sp_a, sp_b, sp_ds, x, m, dm, hd2);
                    const double S = OWN ? fma(own1, x, pend[e][0] + m) : pend[e][0] + m;
                    // m'(x); x 0: a NaN / infinite sample stays NaN beside a constant slope
                    const double m1 = OWN ? fma(dm, sp_ds, fma(x, 0.0, own1)) : dm * sp_ds;
                    double n1 = m1;
                    if (af) {                                 // the log-determinant term at t: a second gather
                        const double t = fma(t_a, x, t_b);
                        double mt, dmt = 0.0;
                        hd2 = 0.0;
                        if (nI > 0) band_spline_d2<false>(tab, nI, sp_a, sp_b, sp_ds, t, mt, dmt, hd2);
                        n1 = OWN ? fma(dmt, sp_ds, fma(t, 0.0, own1)) : dmt * sp_ds;
                    }
#pragma unroll
                    for (int l = LAG; l >= 1; --l) acc[e][l] = fma(-(gl[l] * S), dq[e][l * (l - 1) / 2 + l - 1], acc[e][l - 1]);
                    acc[e][0] = fma(-(gl[0] * S), m1, band_div(hd2 * c2, n1));
                    xr[e] = x;
                    Er[e] = band_expq(etab, x, kt);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    if (j >= LAG) store(j - LAG, q, acc[2 * q][LAG], acc[2 * q + 1][LAG]);
                // group by group (one group's coefficients in scalar registers at a time): the pushes of band_push and the groups'
                // derivatives, which go to the head of their queues
#pragma unroll
                for (int l = 0; l < LAG; ++l) {
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        double dnew;
                        pend[e][l] = band_group_d<DB, DA>(rec + TTM_P_HDR + l * GP, l + 1 < LAG ? pend[e][l + 1] : start, xr[e], -0.5 * xr[e], Er[e], dnew);
#pragma unroll
                        for (int a = l; a >= 1; --a) dq[e][(l + 1) * l / 2 + a] = dq[e][(l + 1) * l / 2 + a - 1];
                        dq[e][(l + 1) * l / 2] = dnew;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                rec += PS; xcol += ldxb;
            };
            int j = kb;
            for (; j + 1 < ke; j += 2) {
                step(j, xa, xb);
                step(j + 1, xb, xa);
            }
            if (j < ke) step(j, xa, xb);
        }
        // the last LAG columns: nothing beyond component D - 1 contributes
#pragma unroll
        for (int l = 0; l < LAG; ++l) {
            if (D - 1 - l >= 0) {
#pragma unroll
                for (int q = 0; q < NP; ++q) store(D - 1 - l, q, acc[2 * q][l], acc[2 * q + 1][l]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// TEST HOOK (ttm_math_probe, include/ttm.h): the primitives of this file on arrays, one element per thread - the pair table
// staged by the loader of k_band_forward, the Taylor coefficients read as the kernels read them.  No map kernel calls this.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BAND_CT) void k_band_math_probe(int which, const double* __restrict__ a, const double* __restrict__ b,
                                                             int64_t n, double* __restrict__ out) {
    extern __shared__ __align__(16) double g_lds[];
    double* etab = g_lds;
    band_stage(etab, g_band_etab, 2 * TTM_BAND_ET_N);
    __syncthreads();
    cdbl_p kt = (cdbl_p)g_band_taylor;
    const int64_t i = (int64_t)blockIdx.x * BAND_CT + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    double r;
    switch (which) {
        case TTM_PROBE_BAND_EXPQ: r = band_expq(etab, x, kt); break;
        case TTM_PROBE_BAND_EXPQ_SERIES: r = band_expq_series(x); break;
        case TTM_PROBE_BAND_EXPQ_FAR: r = band_expq_far(etab, x, kt); break;
        case TTM_PROBE_BAND_LOG: r = band_log(x); break;
        default: r = band_div(x, b[i]); break;
    }
    out[i] = r;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static_assert(BAND_RT_KMAX == BAND_RING_KMAX, "k_band_inverse and the ring plan (ttm_band_image.h) cap a block at the same number of components");

static void allow_lds(const void* kern, size_t bytes) {
    static thread_local const void* seen[16];
    static thread_local size_t granted[16];
    static thread_local int n = 0;
    for (int i = 0; i < n; ++i)
        if (seen[i] == kern) {
            if (granted[i] >= bytes) return;
            granted[i] = bytes;
            (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            return;
        }
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (n < 16) { seen[n] = kern; granted[n] = bytes; ++n; }
}

// the tail of every entry point: BAND_CT threads per workgroup, `lds` bytes of dynamic LDS, the kernel's name for the caller
template <class... P, class... A>
static int launch(void (*kern)(P...), int64_t grid, size_t lds, void* stream, const char* name, const char** kernel_name, A... args) {
    allow_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BAND_CT), lds, (hipStream_t)stream, static_cast<P>(args)...);
    if (kernel_name) *kernel_name = name;
    return 0;
}

// ---- a run-time value picks a template argument: f gets it as a std::integral_constant and returns the kernel.  Every entry
// point has checked the ranges (usable(); the long kernels exist for lag 2 and the classes 1..3 only) ----
template <int V> using int_c = std::integral_constant<int, V>;
template <int NCLS, class F> static auto with_cls(int cls, F f) {          // degree class 1..NCLS (3: the long kernels, 4: the few-component ones)
    if (cls == 1) return f(int_c<1>{});
    if (cls == 2) return f(int_c<2>{});
    if constexpr (NCLS == 4) { if (cls != 3) return f(int_c<4>{}); }
    return f(int_c<3>{});
}
template <class F> static auto with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static auto with_lag(int lag, F f) {                    // groups per push record
    return lag == 5 ? f(int_c<5>{}) : lag == 3 ? f(int_c<3>{}) : f(int_c<2>{});
}
// (record lag, reach of the sweep) of the few-component kernels: exactly the pairs they exist for.  Records of five groups - the
// smoother's block map - have one shape, zeros beyond a sweep's reach
template <class F> static auto with_reach(int lag, int lage, F f) {
    if (lag == 5) return f(int_c<5>{}, int_c<5>{});
    if (lag == 3) return lage == 1 ? f(int_c<3>{}, int_c<1>{}) : lage == 2 ? f(int_c<3>{}, int_c<2>{}) : f(int_c<3>{}, int_c<3>{});
    return lage == 1 ? f(int_c<2>{}, int_c<1>{}) : f(int_c<2>{}, int_c<2>{});
}

// ---- buffers ----
static bool vec_ok(const void* ptr) { return (uintptr_t)ptr % 16 == 0; }   // 16-byte accesses (a null pointer passes: optional buffers)
// a column-major matrix the kernels read and write two rows at a time; need: (N + 1) & ~1 rows per column, or 0 where the
// leading dimension is not held against N
static bool col_ok(const void* ptr, int64_t ld, int64_t need) { return vec_ok(ptr) && ld % 2 == 0 && ld >= need; }
static int64_t even_rows(int64_t N) { return (N + 1) & ~(int64_t)1; }
// the table lookups take exp(w) from its Taylor polynomial: |w| <= 0.1 over the tables' range
static bool y_affine_ok(const double* y) {
    if (!y) return false;
    const double ymax = fabs(y[0]) > fabs(y[2]) ? fabs(y[0]) : fabs(y[2]);
    return y[1] > 0.0 && y[1] * ymax * 0.5 <= 0.1;
}

// ---- grids ----
// rows of a workgroup's chunk: N / #CUs rounded up to whole 128-byte lines of a column, so that every wave's 1 KB
// accesses are line-aligned (a chunk that starts inside a line makes every wave's store touch nine lines, two of them
// partially: the column stream then runs at 72 % of the copy rate instead of ...: profiles/r03_*)
static int64_t chunk_rows(int64_t N, int cus) { return band_policy_chunk_rows(N, cus); }
struct ChunkGrid { int64_t rows, grid; };            // the long kernels: one chunk of rows per workgroup
static ChunkGrid chunk_grid(int64_t N, int cus) {
    const int64_t rows = chunk_rows(N, cus);
    return {rows, (N + rows - 1) / rows};
}
// k_band_forward and k_band_inverse_ring: whole tiles where they keep the CUs busy (band_policy_cut), else the cut above

int record_stride(int cls, int lag) { return rec_stride(cls, lag); }

bool usable(const ttm_program* p, int k0, int k1) {
    return p && p->u_enabled && (p->u_p_lag == 2 || ((p->u_p_lag == 3 || p->u_p_lag == TTM_P_LAG_MAX) && p->D <= TTM_P_FEW_D)) && p->u_h_cls >= 1 &&
           (p->u_h_cls <= 3 || (p->u_h_cls == 4 && p->D <= TTM_P_FEW_D)) &&
           p->h_ucomp && k0 >= 0 && k1 <= p->D && k0 < k1 && p->u_p_stride == rec_stride(p->u_h_cls, p->u_p_lag);
}

static int uc(const ttm_program* p, int k, int word) { return p->h_ucomp[k * TTM_UC_LEN + word]; }

int build_records(const ttm_program* p, double* U, void* stream) {
    if (!p || !p->u_enabled || p->u_p_lag <= 0 || p->u_h_cls <= 0) return 0;
    hipLaunchKernelGGL(k_band_records, dim3(p->D + p->u_p_lag), dim3(64), 0, (hipStream_t)stream, p->ucomp, p->ugrp, U, (int64_t)p->u_h_off,
                       (int)p->u_h_cls, (int)p->u_h_ng, (int64_t)p->u_p_off, (int)p->u_p_lag, (int)p->u_p_stride, (int)p->D);
    return 0;
}

// does a component of [k0, k1) have a linear term of its own variable (slot [7] of its push record; it may then have no spline)?
// (a map without them takes the instantiations without: no slot [7], no test for a missing spline)
static bool sweep_has_own(const ttm_program* p, int k0, int k1) {
    for (int k = k0; k < k1; ++k)
        if (uc(p, k, TTM_UC_FLAGS) & TTM_UCF_OWN) return true;
    return false;
}

// ---- the few-component kernels (k_band_few*): everything requested at once, tiles of 2048 rows, a persistent grid ----
struct FewSweep {
    int tab0, ntab;                                  // the splines of the sweep as they stand in the U section (padding between them included)
    bool stageable;                                  // ... and a launch can stage them: whole 16-byte units, two loads per thread
    size_t lds;                                      // exp table + splines (+ one unit)
    int lage; bool plain;                            // how far back the groups reach; does any of them have plain polynomial terms?
    int64_t ntiles, grid;
};
static FewSweep few_sweep(const ttm_program* p, int k0, int k1, int64_t N, int cus) {
    FewSweep s;
    s.tab0 = uc(p, k0, TTM_UC_TAB_OFF);
    s.ntab = uc(p, k1 - 1, TTM_UC_TAB_OFF) + TTM_U_TSTRIDE * uc(p, k1 - 1, TTM_UC_NI) - s.tab0;
    if (s.ntab <= 0) { s.tab0 = 0; s.ntab = 2; }     // (no spline in the sweep - linear monotone parts: two doubles of the U section stand in)
    s.stageable = s.ntab >= 2 && s.ntab % 2 == 0 && s.tab0 % 2 == 0 && s.ntab <= BAND_FEW_TAB;
    s.lds = ((size_t)BAND_ET_DOUBLES + (size_t)s.ntab + 2) * 8;
    s.lage = 1; s.plain = false;
    for (int k = k0; k < k1; ++k)
        for (int g = 0; g < uc(p, k, TTM_UC_N_GRP); ++g) {
            const int32_t* G = p->h_ugrp + (uc(p, k, TTM_UC_GRP_OFF) + g) * TTM_UG_LEN;
            const int lag = uc(p, k, TTM_UC_KC) - G[TTM_UG_VAR];
            s.lage = lag > s.lage ? lag : s.lage;
            s.plain = s.plain || (G[TTM_UG_FLAGS] & TTM_UGF_POLY);
        }
    const int64_t trows = BAND_FEW_NS * BAND_CT;
    s.ntiles = (N + trows - 1) / trows;
    s.grid = s.ntiles < cus ? s.ntiles : cus;
    return s;
}

// ---- the long kernels: blocks of components whose splines are resident at a time ----
// components per block so that the splines of a block fit `budget` bytes (0: not even one).  A sweep without any spline
// (linear monotone parts) is one block that stages nothing.  `block` > 0: at most that many.
static int plan_blocks(const ttm_program* p, int k0, int k1, size_t budget, int block) {
    auto bytes = [&](int k) { return (size_t)uc(p, k, TTM_UC_NI) * TTM_U_TSTRIDE * 8; };
    const int ncomp = k1 - k0;
    size_t worst = 0;
    for (int k = k0; k < k1; ++k) worst = bytes(k) > worst ? bytes(k) : worst;
    if (worst > budget) return 0;
    for (int nblk = 1; nblk <= ncomp; ++nblk) {
        const int Bc = worst == 0 ? ncomp : (ncomp + nblk - 1) / nblk;
        bool ok = true;
        for (int kb = k0; kb < k1 && ok; kb += Bc) {
            size_t s = 0;
            for (int k = kb; k < kb + Bc && k < k1; ++k) s += bytes(k);
            ok = s <= budget;
        }
        if (ok) return block > 0 && block < Bc ? block : Bc;
    }
    return 0;
}
// Dynamic LDS of the splines under a plan of Bc components per block, the largest block's.  Two rules, kept apart on purpose:
// by SUM of the components' splines - how forward() sizes k_band_forward and k_band_density
static size_t block_lds_sum(const ttm_program* p, int k0, int k1, int Bc) {
    size_t lds = 0;
    for (int kb = k0; kb < k1; kb += Bc) {
        size_t s = 0;
        for (int k = kb; k < kb + Bc && k < k1; ++k) s += (size_t)uc(p, k, TTM_UC_NI) * TTM_U_TSTRIDE * 8;
        lds = s > lds ? s : lds;
    }
    return lds;
}
// by SPAN, from the block's first spline to the end of its last as they stand in the U section - what k_band_search stages
// (from its first component's offset, spline or not) and k_band_logdet (`splines_only`: from the first component that has one)
static size_t block_lds_span(const ttm_program* p, int k0, int k1, int Bc, bool splines_only) {
    size_t lds = 0;
    for (int kb = k0; kb < k1; kb += Bc) {
        int a = kb, b = (kb + Bc < k1 ? kb + Bc : k1) - 1;
        if (splines_only) {
            while (a <= b && uc(p, a, TTM_UC_NI) <= 0) ++a;
            while (b >= a && uc(p, b, TTM_UC_NI) <= 0) --b;
        }
        const size_t s = a > b ? 0 : (size_t)(uc(p, b, TTM_UC_TAB_OFF) + TTM_U_TSTRIDE * uc(p, b, TTM_UC_NI) - uc(p, a, TTM_UC_TAB_OFF)) * 8;
        lds = s > lds ? s : lds;
    }
    return lds;
}

int forward(const ttm_program* p, const double* U, int k0, int k1, const double* Xsoa, int64_t ldx, int64_t N, double* Zsoa, int64_t ldz,
            double* logdet, const double* sigma, double* sumsq, int cus, size_t lds_per_cu, int block, int resident, int full_tiles,
            void* stream, const char** kernel_name) {
    // (rows: 2^28 here, 2^29 at the gate in ttm_kernels.hip - both stand)
    if (!usable(p, k0, k1) || (!Zsoa && !logdet && !sumsq) || N >= ((int64_t)1 << 28)) return 1;
    // (need = 0 for Z: ldz is not held against N here, as it is in roundtrip() and newton())
    if (!col_ok(Xsoa, ldx, even_rows(N)) || (Zsoa && !col_ok(Zsoa, ldz, 0)) || !vec_ok(U) || !vec_ok(logdet) || !vec_ok(sumsq)) return 1;
    const bool dens = logdet || sumsq;
    const size_t stat = dens ? (size_t)BAND_UNI * 8 : 0;                                 // (static array of the density pass)
    if (dens && k1 - k0 > BAND_UNI) return 1;
    const size_t fixed = (size_t)BAND_ET_DOUBLES * 8 + stat;
    if (lds_per_cu <= fixed) return 1;
    const int Bc = plan_blocks(p, k0, k1, lds_per_cu - fixed, block);
    if (Bc <= 0) return 1;
    const size_t lds = block_lds_sum(p, k0, k1, Bc) + fixed - stat;                      // (dynamic part)
    const int cls = p->u_h_cls, lag = p->u_p_lag, kcol0 = uc(p, k0, TTM_UC_KC);
    // log-determinant only: the derivative of a separable component is a function of its own column alone (k_band_logdet)
    if (logdet && !Zsoa && !sumsq && k1 - k0 <= BAND_UNI) {
        const size_t lbudget = lds_per_cu - (size_t)BAND_UNI * 8;
        const int LBc = plan_blocks(p, k0, k1, lbudget, block);
        const size_t llds = LBc > 0 ? block_lds_span(p, k0, k1, LBc, true) + 16 : 0;
        if (LBc > 0 && llds <= lbudget) {
            const ChunkGrid cg = chunk_grid(N, cus);
            auto lk = with_lag(lag, [&](auto L) {
                return with_bool(cg.rows >= 3 * BAND_CT, [&](auto wide) { return k_band_logdet<decltype(L)::value, decltype(wide)::value ? 4 : 2>; });
            });
            return launch(lk, cg.grid, llds, stream, "k_band_logdet", kernel_name, U, p->u_p_off, k0, k1, kcol0, p->u_p_stride, Xsoa, ldx, N, logdet,
                          sigma, cg.rows, LBc);
        }
    }
    // a few components (k_band_few).  A sweep that reaches further back than its records declines outright; any other
    // condition that fails leaves the map to the long kernels below
    if (k1 - k0 <= TTM_P_FEW_D) {
        const FewSweep fs = few_sweep(p, k0, k1, N, cus);
        if (fs.stageable && fs.lds <= lds_per_cu && (!sigma || logdet)) {
            if (fs.lage > lag) return 1;
            auto fk = with_reach(lag, fs.lage, [&](auto L, auto E) {
                return with_bool(fs.plain, [&](auto PL) {
                    return with_bool(dens, [&](auto DN) {
                        return with_cls<4>(cls, [&](auto C) {
                            return k_band_few<decltype(C)::value, decltype(L)::value, decltype(E)::value, decltype(PL)::value, decltype(DN)::value>;
                        });
                    });
                });
            });
            return launch(fk, fs.grid, fs.lds, stream, dens ? "k_band_few<density>" : "k_band_few", kernel_name, U, p->u_p_off, k0, k1, kcol0, Xsoa,
                          ldx, N, Zsoa, ldz, logdet, sigma, sumsq, fs.ntiles, fs.tab0, fs.ntab);
        }
    }
    if (lag != 2 || cls > 3) return 1;                        // (lag-3 records / order class 4: the few-component kernels only)
    const bool own = sweep_has_own(p, k0, k1);
    const ChunkGrid cg = chunk_grid(N, cus);
    if (dens) {
        auto dk = with_bool(Zsoa != nullptr, [&](auto WZ) {
            return with_bool(own, [&](auto OW) {
                return with_cls<3>(cls, [&](auto C) { return k_band_density<decltype(C)::value, 2, decltype(WZ)::value, decltype(OW)::value>; });
            });
        });
        return launch(dk, cg.grid, lds, stream, "k_band_density", kernel_name, U, p->u_p_off, k0, k1, kcol0, Xsoa, ldx, N, Zsoa, ldz, logdet, sigma,
                      sumsq, cg.rows, Bc);
    }
    // the cache policy of the column streams (ttm_band_policy.h): a function of the sizes, or the option's
    const BandCut lc = band_policy_cut(N, cus, full_tiles);   // (whole tiles where they keep the CUs busy, else cg)
    const bool pol = (band_resident_policy(N, lc.rows, k1 - k0, resident) & BAND_POLICY_FORWARD) != 0;
    auto kern = with_bool(pol, [&](auto PO) {
        return with_bool(own, [&](auto OW) {
            return with_cls<3>(cls, [&](auto C) { return k_band_forward<decltype(C)::value, 2, decltype(OW)::value, decltype(PO)::value ? 1 : 0>; });
        });
    });
    return launch(kern, lc.grid, lds, stream, "k_band_forward", kernel_name, U, p->u_p_off, k0, k1, kcol0, Xsoa, ldx, N, Zsoa, ldz, lc.rows, Bc);
}

// forward (+ density terms) + table inverse of a map of a few components in one launch (k_band_few_roundtrip); 1: not for this map /
// these buffers (the caller makes the separate calls)
int roundtrip(const ttm_program* p, const double* U, int k0, int k1, const double* Xsoa, int64_t ldx, int64_t N, double* Zsoa, int64_t ldz,
              double* Xr, int64_t ldr, double* logdet, const double* sigma, double* sumsq, const double* tab_x, int T, const double* y_affine,
              const double* tmin, const double* tmax, const int32_t* bkt, int nb, int cus, size_t lds_per_cu, bool force, void* stream,
              const char** kernel_name) {
    const int nc = k1 - k0;
    if (!usable(p, k0, k1) || nc > TTM_P_FEW_D || !Xr || T < 64 || T + 4 > BAND_CT || nb + 1 != 1024 || N >= ((int64_t)1 << 28)) return 1;
    if (!vec_ok(bkt) || (sigma && !logdet) || !y_affine_ok(y_affine)) return 1;
    const int64_t need = even_rows(N);
    if (!col_ok(Xsoa, ldx, need) || (Zsoa && !col_ok(Zsoa, ldz, need)) || !col_ok(Xr, ldr, need) || !vec_ok(U) || !vec_ok(logdet) || !vec_ok(sumsq))
        return 1;
    const FewSweep fs = few_sweep(p, k0, k1, N, cus);
    const BandImageSlot slot = band_image_slot(T, nb);
    const size_t lds = slot.lds(nc) + fs.lds;
    if (!fs.stageable || lds > lds_per_cu || fs.lage > p->u_p_lag) return 1;
    const bool dens = logdet || sumsq;
    // Where it pays (measured, graph replay): sweeps that reach one or two columns back, without the density terms - C2b 19.9 us
    // against 10.1 + 11.8 us.  A reach of three columns (C3: 29.8 against 10.5 + 13.1 us) and the density variant (C2b 31.6
    // against 15.9 + 11.8 us) run out of registers (34-117 spilled with the inverse sweep's 128 in use): the launches are bound by the
    // latency of a row's chain of dependent operations, not by the columns' traffic, so one pass instead of two saves a launch
    // floor and a round trip, not the arithmetic.  `force`: tests (every shape through the fused kernel).
    if (!force && (fs.lage > 2 || dens)) return 1;
    auto rk = with_reach(p->u_p_lag, fs.lage, [&](auto L, auto E) {
        return with_bool(fs.plain, [&](auto PL) {
            return with_bool(dens, [&](auto DN) {
                return with_cls<4>(p->u_h_cls, [&](auto C) {
                    return k_band_few_roundtrip<decltype(C)::value, decltype(L)::value, decltype(E)::value, decltype(PL)::value, decltype(DN)::value>;
                });
            });
        });
    });
    return launch(rk, fs.grid, lds, stream, dens ? "k_band_few_roundtrip<density>" : "k_band_few_roundtrip", kernel_name, U, p->u_p_off, k0, k1,
                  uc(p, k0, TTM_UC_KC), Xsoa, ldx, N, Zsoa, ldz, Xr, ldr, logdet, sigma, sumsq, tab_x, T, y_affine[0], y_affine[1], y_affine[2], tmin,
                  tmax, bkt, nb, slot.tab_slot, fs.ntiles, fs.tab0, fs.ntab);
}

// root search in push form, planned once for both methods (BIS: the reference's bisection, reported as k_band_few_bisect /
// k_band_bisect; else the Newton search, reported as k_band_few_newton / k_band_newton - instantiations of k_band_few_search /
// k_band_search); 1: not for this map / these buffers (the caller launches the generic kernel)
template <bool BIS>
static int root_search(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
                       int32_t* iters, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name, bool dry = false) {
    if (!usable(p, k0, k1) || !iters || N < 1 || N >= ((int64_t)1 << 28) || cus < 1) return 1;
    if (!col_ok(Zsoa, ldz, even_rows(N)) || !col_ok(Xsoa, ldx, even_rows(N)) || !vec_ok(U)) return 1;
    const int cls = p->u_h_cls, lag = p->u_p_lag, kcol0 = uc(p, k0, TTM_UC_KC);
    if (k1 - k0 <= TTM_P_FEW_D) {
        const FewSweep fs = few_sweep(p, k0, k1, N, cus);
        // (a sweep that reaches further back than its records falls through to the checks of the long kernel; it does not return)
        if (fs.stageable && fs.lds <= lds_per_cu && fs.lage <= lag) {
            auto fk = with_lag(lag, [&](auto L) {
                return with_cls<4>(cls, [&](auto C) { return k_band_few_search<decltype(C)::value, decltype(L)::value, BIS>; });
            });
            if (dry) return 0;                                // (planned: the caller asks before it launches anything)
            return launch(fk, fs.grid, fs.lds, stream, BIS ? "k_band_few_bisect" : "k_band_few_newton", kernel_name, U, p->u_p_off, k0, k1, kcol0, Zsoa,
                          ldz, Xsoa, ldx, N, iters, fs.ntiles, fs.tab0, fs.ntab);
        }
    }
    if (lag != 2 || cls > 3) return 1;                        // (lag-3 records / order class 4: the few-component kernel only)
    const size_t fixed = (size_t)BAND_ET_DOUBLES * 8;
    if (lds_per_cu <= fixed) return 1;
    const int Bc = plan_blocks(p, k0, k1, lds_per_cu - fixed, block);                    // (the residency plan of forward())
    if (Bc <= 0) return 1;
    const size_t lds = block_lds_span(p, k0, k1, Bc, false) + fixed;
    if (lds > lds_per_cu) return 1;
    if (dry) return 0;
    const ChunkGrid cg = chunk_grid(N, cus);
    auto kern = with_bool(sweep_has_own(p, k0, k1), [&](auto OW) {
        return with_cls<3>(cls, [&](auto C) { return k_band_search<decltype(C)::value, 2, decltype(OW)::value, BIS>; });
    });
    return launch(kern, cg.grid, lds, stream, BIS ? "k_band_bisect" : "k_band_newton", kernel_name, U, p->u_p_off, k0, k1, kcol0, Zsoa, ldz, Xsoa, ldx,
                  N, iters, cg.rows, Bc);
}

int newton(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
           int32_t* iters, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name) {
    return root_search<false>(p, U, k0, k1, Zsoa, ldz, Xsoa, ldx, N, iters, cus, lds_per_cu, block, stream, kernel_name);
}

int bisect(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
           int32_t* iters, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name) {
    return root_search<true>(p, U, k0, k1, Zsoa, ldz, Xsoa, ldx, N, iters, cus, lds_per_cu, block, stream, kernel_name);
}

// would bisect() take these buffers?  Every check of bisect(), no launch
bool bisect_plans(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
                  int32_t* iters, int cus, size_t lds_per_cu, int block) {
    return root_search<true>(p, U, k0, k1, Zsoa, ldz, Xsoa, ldx, N, iters, cus, lds_per_cu, block, nullptr, nullptr, true) == 0;
}

constexpr double BAND_WFRAC = 0.52;                  /* fraction of a table's grid points a window keeps (k_inverse_rt) */

// resident-table images (ttm_band_image.h) of the components [k0, k1) for this table geometry: the plan, or false
bool image_plan(const ttm_program* p, int k0, int k1, int T, int nb, size_t lds_per_cu, int window, int block, int slopes, int* w0, int* W,
                int* tab_slot) {
    if (!usable(p, k0, k1) || p->u_p_lag != 2 || k1 - k0 <= TTM_P_FEW_D) return false;
    BandRingPlan pl;
    if (!band_ring_plan(T, nb, k1 - k0, lds_per_cu, window, block, BAND_WFRAC, &pl, slopes)) return false;
    *w0 = pl.w0; *W = pl.W; *tab_slot = pl.tab_slot;
    return true;
}

// k_band_inverse: whole blocks of Bc tables [w0, w0 + W) resident at a time (+ a short block: the kernel staggers them); Bc = 0: none fits
struct BlockPlan { int W, w0, tab_slot, Bc, nblk; size_t lds; };
static BlockPlan block_plan(int T, int W, int nb, int ncomp, size_t lds_per_cu, int block) {
    const BandImageSlot slot = band_image_slot(W, nb);
    BlockPlan b = {W, (T - W) / 2, slot.tab_slot, 0, 0, 0};
    if (slot.lds(1) > lds_per_cu) return b;
    b.Bc = (int)((lds_per_cu - slot.lds(0)) / ((size_t)slot.tab_slot * 8));
    if (b.Bc > ncomp) b.Bc = ncomp;
    if (b.Bc > BAND_RT_KMAX) b.Bc = BAND_RT_KMAX;
    if (block > 0 && block < b.Bc) b.Bc = block;
    b.nblk = (ncomp + b.Bc - 1) / b.Bc;
    b.lds = slot.lds(b.Bc);
    return b;
}

// table inverse, in this order: the few-component kernel, the ring kernel (images at hand, laid out for this very plan), the block kernel
int inverse(const ttm_program* p, const double* U, int k0, int k1, const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N,
            const double* tab_x, int T, const double* y_affine, const double* tmin, const double* tmax, const int32_t* bkt, int nb, const double* img,
            int img_doubles, int cus, size_t lds_per_cu, int window, int block, int resident, int full_tiles, int zdma, int ring_slots,
            int slopes, void* stream, const char** kernel_name) {
    if (!usable(p, k0, k1) || T < 64 || T > 4096 || nb + 1 != 1024 || N >= ((int64_t)1 << 28)) return 1;      // (bucket rows copied 16 bytes at a time, 256 units per row)
    if (!vec_ok(bkt) || !y_affine_ok(y_affine)) return 1;
    if (!col_ok(Zsoa, ldz, even_rows(N)) || !col_ok(Xsoa, ldx, even_rows(N))) return 1;
    const int ncomp = k1 - k0, cls = p->u_h_cls, lag = p->u_p_lag, kcol0 = uc(p, k0, TTM_UC_KC);
    // a few components: whole tables, everything requested at once, tiles of 2048 rows
    if (ncomp <= TTM_P_FEW_D && T + 4 <= BAND_CT && window <= 0) {          // (no blocks, no windows: `block` does not apply)
        const BandImageSlot slot = band_image_slot(T, nb);
        const FewSweep fs = few_sweep(p, k0, k1, N, cus);
        // (a sweep that reaches further back than its records falls through to the checks below; it does not return)
        if (slot.lds(ncomp) <= lds_per_cu && fs.lage <= lag) {
            auto fk = with_reach(lag, fs.lage, [&](auto L, auto E) {
                return with_bool(fs.plain, [&](auto PL) {
                    return with_cls<4>(cls, [&](auto C) {
                        return k_band_few_inverse<decltype(C)::value, decltype(L)::value, decltype(E)::value, decltype(PL)::value>;
                    });
                });
            });
            return launch(fk, fs.grid, slot.lds(ncomp), stream, "k_band_few_inverse", kernel_name, U, p->u_p_off, k0, k1, kcol0, Zsoa, ldz, Xsoa, ldx,
                          N, tab_x, T, y_affine[0], y_affine[1], y_affine[2], tmin, tmax, bkt, nb, slot.tab_slot, fs.ntiles);
        }
    }
    if (lag != 2 || cls > 3) return 1;                        // (lag-3 records / order class 4: the few-component kernels only)
    const ChunkGrid cg = chunk_grid(N, cus);
    // resident-table images at hand (ttm_inverse_table_build_index wrote them): the ring kernel
    BandRingPlan pl;
    bool ring = img && vec_ok(img) && band_ring_plan(T, nb, ncomp, lds_per_cu, window, block, BAND_WFRAC, &pl, slopes);
    // a coefficient vector's images follow the value of band_slopes they were built under: the doubles per image tell the layout
    // (an image with slopes is larger than any image without under the same window option), so the plan of the other value is tried
    // too.  The doubles per image are an exact signature only while rt_window stays what it was at the build: an image without
    // slopes of a window with Weven = 2 Weven' has as many doubles as one with slopes of a window with Weven', so a caller that
    // changes rt_window AND band_slopes between build and lookup in just that ratio would have its images read in the wrong layout
    if (ring && pl.tab_slot != img_doubles) ring = band_ring_plan(T, nb, ncomp, lds_per_cu, window, block, BAND_WFRAC, &pl, pl.slopes ? 0 : 1);
    if (ring && pl.tab_slot == img_doubles) {                 // (laid out for another plan - options changed in between: not this kernel)
        // the cut (as forward()), the cache policy, ZD and the slots of the ring: band_ring_launch, ttm_band_image.h
        const BandRingLaunch rl = band_ring_launch(pl, N, cus, ncomp, lds_per_cu, full_tiles, resident, zdma, ring_slots);
        const BandCut lc = rl.cut;
        const bool pol = rl.pol, zd = rl.zd;
        pl = rl.ring;
        const bool sl = pl.slopes != 0;
        auto rk = with_bool(pl.G == 4, [&](auto G4) {
            return with_cls<3>(cls, [&](auto C) {
                constexpr int CL = decltype(C)::value, GG = decltype(G4)::value ? 4 : 0;
                if (sl) return pol ? k_band_inverse_ring<CL, 2, GG, 1, 0, 1> : k_band_inverse_ring<CL, 2, GG, 0, 0, 1>;   // (never beside ZD: band_ring_launch)
                return zd ? k_band_inverse_ring<CL, 2, GG, 1, 1> : pol ? k_band_inverse_ring<CL, 2, GG, 1> : k_band_inverse_ring<CL, 2, GG>;
            });
        });
        return launch(rk, lc.grid, pl.lds, stream, "k_band_inverse_ring", kernel_name, U, p->u_p_off, k0, k1, kcol0, Zsoa, ldz, Xsoa, ldx, N, tab_x, T,
                      y_affine[0], y_affine[1], y_affine[2], tmin, tmax, img, nb, pl.tab_slot, pl.R, lc.rows, pl.w0, pl.W);
    }
    BlockPlan b = block_plan(T, T, nb, ncomp, lds_per_cu, block);
    // windowed tables when that saves a pass over the chunk (k_inverse_rt): on request (window > 0: whenever they fit), or by
    // default (window < 0) when whole tables need several blocks and windowed ones fewer
    if (window != 0 && (window > 0 || (b.Bc > 0 && b.nblk > 1))) {
        int W = window > 0 ? (window < 16 ? 16 : window) : (int)(BAND_WFRAC * T);
        if (W >= T) W = T - 1;
        const BlockPlan w = block_plan(T, W, nb, ncomp, lds_per_cu, block);
        if (w.Bc > 0 && (window > 0 || w.nblk < b.nblk)) b = w;
    }
    if (b.Bc <= 0) return 1;
    auto kern = with_cls<3>(cls, [&](auto C) { return k_band_inverse<decltype(C)::value, 2, BAND_RT_KMAX>; });
    return launch(kern, cg.grid, b.lds, stream, "k_band_inverse", kernel_name, U, p->u_p_off, k0, k1, kcol0, Zsoa, ldz, Xsoa, ldx, N, tab_x, T,
                  y_affine[0], y_affine[1], y_affine[2], tmin, tmax, bkt, nb, b.tab_slot, b.Bc, cg.rows, b.w0, b.W);
}

// score of the pullback density of the whole map in push form (k_band_score): the residency plan of the root searches, one
// kernel body for every degree class, record lag and own-term shape; 1: not for this map / these buffers (the caller launches
// the generic kernel)
int score(const ttm_program* p, const double* U, const double* Xsoa, int64_t ldx, int64_t N, double* Gsoa, int64_t ldg, const double* g_scale,
          const double* ld_affine, int cus, size_t lds_per_cu, int block, void* stream, const char** kernel_name) {
    if (!p || !usable(p, 0, p->D) || !Xsoa || !Gsoa || N < 1 || N >= ((int64_t)1 << 28) || cus < 1) return 1;
    if (!col_ok(Xsoa, ldx, even_rows(N)) || !col_ok(Gsoa, ldg, even_rows(N)) || !vec_ok(U)) return 1;
    const int D = p->D, cls = p->u_h_cls, lag = p->u_p_lag, kcol0 = uc(p, 0, TTM_UC_KC);
    const size_t fixed = (size_t)BAND_ET_DOUBLES * 8;
    if (lds_per_cu <= fixed) return 1;
    const int Bc = plan_blocks(p, 0, D, lds_per_cu - fixed, block);
    if (Bc <= 0) return 1;
    const size_t lds = block_lds_span(p, 0, D, Bc, false) + fixed;
    if (lds > lds_per_cu) return 1;
    const ChunkGrid cg = chunk_grid(N, cus);
    auto kern = with_lag(lag, [&](auto L) {
        return with_bool(sweep_has_own(p, 0, D), [&](auto OW) {
            return with_cls<4>(cls, [&](auto C) { return k_band_score<decltype(C)::value, decltype(L)::value, decltype(OW)::value>; });
        });
    });
    allow_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)cg.grid), dim3(band_score_ct(cls, lag)), lds, (hipStream_t)stream, U, (int64_t)p->u_p_off, D, kcol0, Xsoa, ldx, N,
                       Gsoa, ldg, g_scale, ld_affine, (int64_t)cg.rows, Bc);
    if (kernel_name) *kernel_name = "k_band_score";
    return 0;
}

int math_probe(int which, const double* a, const double* b, int64_t n, double* out, void* stream, const char** kernel_name) {
    return launch(k_band_math_probe, (n + BAND_CT - 1) / BAND_CT, (size_t)BAND_ET_DOUBLES * 8, stream, "k_band_math_probe", kernel_name, which, a, b,
                  n, out);
}

}  // namespace ttm_band
