// ttm_options.h - the launch-planning options (include/ttm.h: ttm_set_option), shared by libttm.so and the host test
// double (tests/hostemu/ttm_hostemu.cpp), so that both accept and reject the same names.  Plain C++.
#pragma once

#include <string.h>

// Options: what a test or a tuning run may override (ttm_set_option); every process starts from these defaults and
// ttm_reset_options goes back to them.  -1 = "let the launch planning decide".
#define TTM_OPTIONS(X)                                                                                                   \
    X(no_plan, 0)        /* 1: generic kernels instead of the planned-cache ones                                     */ \
    X(no_uform, 0)       /* 1: direct kernels instead of the U-form ones                                             */ \
    X(u_no_hot, 0)       /* 1: U-form kernels without hot records                                                    */ \
    X(u_loader, -1)      /* 0 / 1: loader-wave forward kernels off / on whatever the ensemble size                   */ \
    X(forward_ns, -1)    /* samples per thread of the generic forward kernels (1, 2, 4)                              */ \
    X(inverse_ns, -1)    /* samples per thread of the generic table inverse (1, 2)                                   */ \
    X(u_ns, -1)          /* samples per thread of k_forward_u (1, 2, 4)                                              */ \
    X(hl_ns, -1)         /* samples per evaluating thread of k_forward_hl (2, 4)                                     */ \
    X(rt_off, 0)         /* 1: table inverse through the generic kernel instead of k_inverse_rt                      */ \
    X(rt_ns, -1)         /* rows per thread of k_inverse_rt (2, 4)                                                   */ \
    X(rt_block, -1)      /* components per block of k_inverse_rt                                                     */ \
    X(rt_band, -1)       /* 0: banded maps through the LDS column cache instead of the register shift                */ \
    X(rt_window, -1)     /* resident entries per table of k_inverse_rt: 0 whole tables, > 0 that many, -1 planned    */ \
    X(gram_mfma, -1)     /* 0: Gram matrices by the pairwise kernel instead of the matrix cores                      */ \
    X(band_fwd, -1)      /* 0: banded maps through k_forward_hl instead of the push-form kernel (csrc/ttm_band.hip)   */ \
    X(band_inv, -1)      /* 0: banded maps through k_inverse_rt instead of the push-form kernel                      */ \
    X(band_cus, -1)      /* > 0: the band kernels plan their row chunks for this many CUs (tests: several tiles per chunk) */ \
    X(band_ring, -1)     /* 0: banded table inverse through k_band_inverse (tables assembled per block) although images are at hand */ \
    X(band_newton, -1)   /* 0: Newton root search of banded maps through the generic k_inverse_newton instead of the push-form kernels */ \
    X(band_bisect, -1)   /* 0: bisection of banded maps (no cap) through the generic k_inverse_bisect instead of the push-form kernels */ \
    X(band_score, -1)    /* 0: the score of banded maps (ttm_score) through the generic k_score_u instead of the push-form kernel   */ \
    X(band_resident, -1) /* cache policy of k_band_forward / k_band_inverse_ring (csrc/ttm_band_policy.h): 0 plain, 1 / 2 / 3 forward / inverse / both keep half of Z on-die */ \
    X(band_full_tiles, -1) /* cut of k_band_forward / k_band_inverse_ring launches (csrc/ttm_band_policy.h): 0 N / #CUs rows per workgroup, 1 whole tiles of 4096 rows wherever they give every CU at most one */ \
    X(band_zdma, -1)     /* k_band_inverse_ring requests Z two columns ahead through LDS on full tiles (ZD = 1, beside the resident policy only): 0 off, 1 wherever it fits */ \
    X(band_ring_slots, -1) /* slots of a refilled ring of k_band_inverse_ring: 0 as many as fit, > 0 at most that many (whole groups of 4, 12 at least) */ \
    X(band_slopes, -1)   /* resident-table images with the slope of every interval, read by k_band_inverse_ring instead of formed per row (csrc/ttm_band_image.h): 0 off, 1 wherever the ring plan allows; images follow the value they were built under */ \
    X(int_dense, -1)     /* 0: integrated maps with dense B sets through the generic kernels instead of csrc/ttm_int.hip */ \
    X(int_xprog, -1)     /* 0: integrated components without their X programs (csrc/ttm_xprog.h: forward map, objective / gradient sums); \
                            2: the root searches through them as well (measured: the weights are 1 % of a bisection - no gain, 5 % slower at C2a) */ \
    X(fold_fused, -1)    /* 0: ttm_fold as three launches (k_fold, k_uform, k_band_records) instead of one                */ \
    X(table_fused, -1)   /* 0: inverse tables as two launches (k_table_build, k_table_index) instead of one               */ \
    X(setup_fused, -1)   /* 0: ttm_setup_staged declines (the caller then launches ttm_fold_staged and the table kernel)           */ \
    X(select_coop, -1)   /* 0: order statistics by 17 launches (k_select_hist / k_select_pick) whatever the column length;         \
                            2: tests - the one-launch select with every wait given up at once (workgroup 0 selects by itself)    */ \
    X(colstats_one, -1)  /* 0: column moments by four launches (k_colsum / k_colfinish) whatever the shape                        */ \
    X(sep_sentinel, -1)  /* 0: the evaluations of ttm_optimize_separable with ticket and completion mark whatever the grid;       \
                            2: tests - the finishing workgroup gives up at once (the failure pattern reaches the host)            */ \
    X(sep_server, -1)    /* 0: the loops of ttm_optimize_separable launch per evaluation instead of ONE evaluation server per loop      */ \
    X(wscan_reread, -1)  /* 1: the last launch of ttm_weight_scan rereads the q its tile-sum launch parked in cum instead of forming exp again */ \
    X(roundtrip_fused, -1) /* 0: ttm_roundtrip declines (the caller makes the forward and the inverse call); 1: the fused kernel for \
                              every shape it can run, also those it is slower for (reach of three columns, density terms)          */

struct Tuning {
#define X(name, dflt) int name = dflt;
    TTM_OPTIONS(X)
#undef X
};

// the field of option `name`, or nullptr for a name that is not an option
static inline int* tuning_field(Tuning& t, const char* name) {
#define X(field, dflt) if (!strcmp(name, #field)) return &t.field;
    TTM_OPTIONS(X)
#undef X
    return nullptr;
}
