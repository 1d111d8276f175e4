// ultr_rowgrad_plan.h - host-only arithmetic of the row-gradient launches (csrc/ultr_rowgrad.hip): how many partials a column-sum job
// and a split-over-rows weight gradient leave for the fold.  The plans of the models that use them (ultr_dlcm_plan.h, ultr_gsf_plan.h)
// size their workspaces with it.
#pragma once
#include <stdint.h>

#define RG_CS_ROWS 256       // rows per partial of the column-sum launch
#define RG_WG_SPLITS 64      // at most this many row splits of a weight-gradient launch

static inline int64_t rg_up4(int64_t n) { return (n + 3) & ~(int64_t)3; }
static inline int64_t rg_cs_chunks(int64_t T) { return (T + RG_CS_ROWS - 1) / RG_CS_ROWS; }
// rows per split of rg_wgrad_kernel: at least 128 (32 matrix-core steps), a multiple of 4, at most RG_WG_SPLITS splits
static inline int64_t rg_wg_chunk(int64_t K) {
  const int64_t c = rg_up4((K + RG_WG_SPLITS - 1) / RG_WG_SPLITS);
  return c < 128 ? 128 : c;
}
static inline int64_t rg_wg_splits(int64_t K) { return K <= 0 ? 0 : (K + rg_wg_chunk(K) - 1) / rg_wg_chunk(K); }
