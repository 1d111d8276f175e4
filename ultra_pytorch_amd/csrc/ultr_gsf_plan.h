// ultr_gsf_plan.h - host-only geometry of the GSF ranking model (csrc/ultr_gsf.hip): parameter offsets, the layout of `saved` / `work` /
// `workspace`, and the shape limits every entry point checks before a launch.  DESIGN.md section 3e.
#pragma once
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_rowgrad_plan.h"

#define GSF_MAX_GROUP 8                   // documents per group (the slots a row of the first product gathers)
#define GSF_MAXL (ULTR_MAX_HIDDEN + 1)    // Linear layers: the hidden ones and the head

struct GsfPlan {
  int F, m, nl, act;        // nl = n_hidden + 1 Linear layers; layer nl - 1 is the head (m outputs)
  int K[GSF_MAXL];          // in-features of Linear_j (K[0] = m F): the width LayerNorm_j normalises
  int M[GSF_MAXL];          // out-features of Linear_j (M[nl - 1] = m)
  int maxK;                 // the widest LayerNorm input
  int64_t off_g[GSF_MAXL], off_b[GSF_MAXL], off_w[GSF_MAXL], off_c[GSF_MAXL], P;  // gamma, beta, weight, bias of layer j (the DNN's order)
  int B, L;
  int64_t T;                // group rows = B L
  // `saved` / `work`: what one launch hands to the next ...
  int64_t s_slots;          // uint32 [T, GSF_MAX_GROUP]: the byte offset of each slot's feature row (ULTR_OOB: a PAD, or no such slot)
  int64_t s_mean[GSF_MAXL], s_rstd[GSF_MAXL];  // [T] each: the statistics of LayerNorm_j
  int64_t s_a[GSF_MAXL];    // [T, M[j]], j < nl - 1: act(Linear_j); the scoring form keeps two of them (even / odd layers)
  int64_t s_o;              // [T, m]: the group outputs
  int64_t score_floats;
  // ... and, in `saved` only, what the backward alone reads
  int64_t s_xhat;           // [T, m F]: the normalised gathered rows (4 m F bytes per group row)
  int64_t saved_floats;
  // `workspace` of the backward
  int64_t w_do;             // [T, m]
  int64_t w_dz[GSF_MAXL];   // [T, M[j]], j < nl - 1: the gradient of Linear_j's output
  int64_t w_du;             // [T, maxK]: the gradient of LayerNorm_j's output, one layer at a time
  int64_t w_cs[GSF_MAXL];   // column-sum partials of layer j: [chunks][M[j] + 2 K[j]]
  int64_t w_wp[GSF_MAXL];   // weight-gradient partials of layer j: [splits][M[j] K[j]]
  int64_t ws_floats;
};

// is it a model at all?  (the parameter layout is defined for every such descriptor, supported by the kernels or not)
static inline bool gsf_is_model(const ultr_gsf_desc* c) {
  if (c == nullptr || c->feature_size <= 0 || c->group_size <= 0 || c->n_hidden < 0 || c->n_hidden > ULTR_MAX_HIDDEN) return false;
  if (c->activation < 0 || c->activation > 3) return false;
  if ((int64_t)c->feature_size * c->group_size > 0x7fffffff) return false;
  for (int j = 0; j < c->n_hidden; ++j)
    if (c->hidden[j] <= 0) return false;
  return true;
}
// 0, ULTR_E_BADARG (not a model) or ULTR_E_UNSUPPORTED (a model these kernels do not take)
static inline int gsf_check_desc(const ultr_gsf_desc* c) {
  if (!gsf_is_model(c)) return ULTR_E_BADARG;
  if (c->group_size > GSF_MAX_GROUP || (c->feature_size & 3) != 0) return ULTR_E_UNSUPPORTED;  // 16-byte rows: ultr_gemm.h's vector loads
  for (int j = 0; j < c->n_hidden; ++j)
    if ((c->hidden[j] & 3) != 0) return ULTR_E_UNSUPPORTED;
  return 0;
}

static inline void gsf_param_layout(const ultr_gsf_desc* c, GsfPlan& p) {
  p.F = c->feature_size; p.m = c->group_size; p.nl = c->n_hidden + 1; p.act = c->activation;
  int k = p.F * p.m;
  int64_t off = 0;
  p.maxK = k;
  for (int j = 0; j < p.nl; ++j) {
    const int mo = j < c->n_hidden ? c->hidden[j] : p.m;
    p.K[j] = k; p.M[j] = mo;
    p.off_g[j] = off; off += k;
    p.off_b[j] = off; off += k;
    p.off_w[j] = off; off += (int64_t)mo * k;
    p.off_c[j] = off; off += mo;
    if (k > p.maxK) p.maxK = k;
    k = mo;
  }
  p.P = off;
}

// the buffers of a call at B lists of L documents (a size query passes its n_rows as T: every B x L = n_rows has the same layout).
// train: the layout of `saved`; otherwise of `work`, whose layer outputs alternate between two buffers.
static inline void gsf_make_plan(const ultr_gsf_desc* c, int64_t B, int64_t L, int64_t T, bool train, GsfPlan& p) {
  gsf_param_layout(c, p);
  p.B = (int)B; p.L = (int)L; p.T = T;
  const int top = p.nl - 1;
  int64_t off = 0;
  p.s_slots = off; off += T * GSF_MAX_GROUP;
  for (int j = 0; j < p.nl; ++j) {
    p.s_mean[j] = off; off += rg_up4(T);
    p.s_rstd[j] = off; off += rg_up4(T);
  }
  if (train) {
    for (int j = 0; j < top; ++j) { p.s_a[j] = off; off += T * p.M[j]; }
  } else {
    int64_t w[2] = {0, 0};
    for (int j = 0; j < top; ++j)
      if (T * p.M[j] > w[j & 1]) w[j & 1] = T * p.M[j];
    for (int j = 0; j < top; ++j) p.s_a[j] = off + (j & 1 ? w[0] : 0);
    off += w[0] + w[1];
  }
  p.s_o = off; off += rg_up4(T * p.m);
  p.score_floats = off;
  p.s_xhat = off; off += T * p.K[0];
  p.saved_floats = off;
  off = 0;
  p.w_do = off; off += rg_up4(T * p.m);
  for (int j = 0; j < top; ++j) { p.w_dz[j] = off; off += T * p.M[j]; }
  p.w_du = off; off += T * p.maxK;
  for (int j = 0; j < p.nl; ++j) {
    p.w_cs[j] = off; off += rg_up4(rg_cs_chunks(T) * (p.M[j] + 2 * (int64_t)p.K[j]));
    p.w_wp[j] = off; off += rg_up4(rg_wg_splits(T) * (int64_t)p.M[j] * p.K[j]);
  }
  p.ws_floats = off;
}

// every buffer a kernel reaches through a buffer resource (or indexes with 32 bits) stays below 2 GiB
static inline bool gsf_sizes_fit(const GsfPlan& p, int64_t n_docs) {
  const int64_t lim = (int64_t)0x7fffffff / 4;
  int64_t widest = p.maxK;
  for (int j = 0; j < p.nl; ++j)
    if (p.M[j] > widest) widest = p.M[j];
  return p.T * widest < lim && n_docs * p.F < lim && p.P < lim && n_docs <= 0x7fffffff;
}
