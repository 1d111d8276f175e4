// ultr_dlcm_plan.h - host-only geometry of the DLCM ranking model (csrc/ultr_dlcm.hip): parameter offsets, the layout of `saved` /
// `work` / `workspace`, the LDS the two recurrent kernels ask for, and the shape limits every entry point checks before a launch.
#pragma once
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_rowgrad_plan.h"

#define DL_LISTS 16         // lists per workgroup of the recurrent kernels = the rows of one 16x16x4 matrix-core tile
#define DL_WAVES 8          // waves per workgroup: column tiles of 16 hidden units are dealt round-robin to them
#define DL_LDS_MAX (160 * 1024)

struct DlPlan {
  int F, H, heads, Hp;      // Hp: H rounded up to the 16-column tile (the padding columns hold zeros)
  int B, L;
  int64_t T, P;
  // parameters (floats into the flat vector, state_dict order)
  int64_t p_gamma, p_beta, p_wih, p_whh, p_bih, p_bhh, p_wphi, p_bphi, p_v;
  // `saved` / `work`: what one launch hands to the next ...
  int64_t s_mean, s_rstd, s_gi, s_o, s_M, s_m, score_floats;
  // ... and, in `saved` only, what the backward alone reads
  int64_t s_xhat, s_gates, saved_floats;
  // `workspace` of the backward
  int64_t w_dgi, w_dgh, w_dxh, w_dM, w_ds, w_dv, w_cspart, w_wpart_ih, w_wpart_hh, w_dh, dh_floats, ws_floats;
  int64_t lds_fwd, lds_bwd;  // bytes
  bool dh_global;            // the backward's carried dh sits in `workspace`: dg and dh do not both fit the LDS
};

// 0, ULTR_E_BADARG (not a model) or ULTR_E_UNSUPPORTED (a model these kernels do not take)
static inline int dl_check_desc(const ultr_dlcm_desc* c) {
  if (c == nullptr || c->feature_size <= 0 || c->hidden_size <= 0 || c->num_heads <= 0) return ULTR_E_BADARG;
  if ((c->feature_size & 3) != 0 || (c->hidden_size & 3) != 0) return ULTR_E_UNSUPPORTED;  // 16-byte rows: ultr_gemm.h's vector loads
  return 0;
}

// parameter offsets alone: defined for every well-formed descriptor, supported by the kernels or not
static inline void dl_param_layout(const ultr_dlcm_desc* c, DlPlan& p) {
  const int64_t F = c->feature_size, H = c->hidden_size, hd = c->num_heads;
  p.F = (int)F; p.H = (int)H; p.heads = (int)hd; p.Hp = (int)((H + 15) / 16 * 16);
  p.p_gamma = 0;
  p.p_beta = F;
  p.p_wih = 2 * F;
  p.p_whh = p.p_wih + 3 * H * F;
  p.p_bih = p.p_whh + 3 * H * H;
  p.p_bhh = p.p_bih + 3 * H;
  p.p_wphi = p.p_bhh + 3 * H;
  p.p_bphi = p.p_wphi + hd * H * H;
  p.p_v = p.p_bphi + hd * H;
  p.P = p.p_v + hd;
}

// the buffers of a call at B lists of L documents (a size query passes its n_rows as both: the bound for every B x L = n_rows)
static inline void dl_make_plan(const ultr_dlcm_desc* c, int64_t B, int64_t L, int64_t T, DlPlan& p) {
  dl_param_layout(c, p);
  const int64_t F = p.F, H = p.H, hd = p.heads;
  p.B = (int)B; p.L = (int)L; p.T = T;
  p.s_mean = 0;
  p.s_rstd = rg_up4(T);
  p.s_gi = 2 * rg_up4(T);
  p.s_o = p.s_gi + T * 3 * H;
  p.s_M = p.s_o + T * H;
  p.s_m = p.s_M + B * hd * H;
  p.score_floats = p.s_m + B * H;
  p.s_xhat = p.score_floats;
  p.s_gates = p.s_xhat + T * F;
  p.saved_floats = p.s_gates + T * 4 * H;
  p.w_dgi = 0;
  p.w_dgh = T * 3 * H;
  p.w_dxh = 2 * T * 3 * H;
  p.w_dM = p.w_dxh + T * F;
  p.w_ds = p.w_dM + B * hd * H;
  p.w_dv = p.w_ds + B * H;
  p.w_cspart = p.w_dv + rg_up4(B * hd);
  p.w_wpart_ih = p.w_cspart + rg_cs_chunks(T) * (6 * H + 2 * F) + rg_cs_chunks(B) * hd * H;
  p.w_wpart_hh = p.w_wpart_ih + rg_wg_splits(T) * 3 * H * F;
  p.w_dh = p.w_wpart_hh + rg_wg_splits(T - 1) * 3 * H * H;
  p.lds_fwd = (int64_t)2 * DL_LISTS * (p.Hp + 8) * 4;
  p.lds_bwd = (int64_t)DL_LISTS * ((3 * p.Hp + 8) + (p.Hp + 8)) * 4;
  p.dh_global = p.lds_bwd > DL_LDS_MAX;
  if (p.dh_global) p.lds_bwd = (int64_t)DL_LISTS * (3 * p.Hp + 8) * 4;
  p.dh_floats = p.dh_global ? (B + DL_LISTS - 1) / DL_LISTS * DL_LISTS * (p.Hp + 8) : 0;
  p.ws_floats = p.w_dh + p.dh_floats;
}

// every buffer a kernel reaches through a buffer resource stays below 2 GiB
static inline bool dl_sizes_fit(const DlPlan& p, int64_t n_docs) {
  const int64_t lim = (int64_t)0x7fffffff / 4;
  return p.T * 4 * p.H < lim && p.T * p.F < lim && n_docs * p.F < lim && p.P < lim && (int64_t)p.B * p.heads * p.H < lim;
}
