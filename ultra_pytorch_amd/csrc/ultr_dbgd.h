// ultr_dbgd.h - what the weight-perturbing learners share (ultr_dbgd.hip: DBGD / MGD, ultr_nsgd.hip: NSGD): the Linear layout of the
// flat DNN vector and the Box-Muller normal of their noise.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"

#define DBGD_TILE_COLS 16  // weight columns per workgroup of dbgd_noise_kernel

struct DbgdLayout {
  int nl;
  int K[ULTR_MAXL], M[ULTR_MAXL];
  int64_t off_ln[ULTR_MAXL], off_w[ULTR_MAXL], off_b[ULTR_MAXL];
  int tiles[ULTR_MAXL];  // workgroups of layer j: ceil(K_j / 16) column tiles + one for the bias and the LayerNorm entries
  int64_t P;
};

// the standard normal of element e of ranker r under counter tag `tag`: Box-Muller on two uniforms of one Philox draw
// (u1 in (0, 1], u2 in [0, 1))
__device__ __forceinline__ float philox_normal(const Philox& rng, int r, int64_t e, uint32_t tag) {
  uint32_t c[4] = {(uint32_t)e, (uint32_t)r, 0u, tag};
  rng(c);
  const float u1 = (float)((c[0] >> 8) + 1u) * (1.0f / 16777216.0f);
  const float u2 = u01(c[1]);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

static inline bool dbgd_layout(const ultr_dbgd_args* a, DbgdLayout* ly) {
  DnnPlan p;
  if (!a->desc || !ultr_make_dnn_plan(a->desc, 0, &p)) return false;
  memset(ly, 0, sizeof(*ly));
  ly->nl = p.nl;
  ly->P = p.P;
  for (int j = 0; j < p.nl; ++j) {
    ly->K[j] = p.K[j];
    ly->M[j] = p.M[j];
    ly->off_ln[j] = p.off_lnw[j];
    ly->off_w[j] = p.off_w[j];
    ly->off_b[j] = p.off_b[j];
    ly->tiles[j] = (p.K[j] + DBGD_TILE_COLS - 1) / DBGD_TILE_COLS + 1;
    if (p.off_lnb[j] != p.off_lnw[j] + p.K[j]) return false;  // gamma | beta adjacent (ranking_model/dnn.py)
  }
  return ly->P == a->n_params;
}

static inline bool dbgd_shape_ok(const ultr_dbgd_args* a) {
  return a && a->n_rankers >= 1 && a->n_rankers + 1 <= ULTR_DBGD_MAX_RANKERS && a->batch > 0 && a->max_candidates > 0 &&
         a->max_candidates <= ULTR_DBGD_MAX_M && a->rank_list_size > 0 && a->rank_list_size <= a->max_candidates &&
         a->n_params > 0;
}
