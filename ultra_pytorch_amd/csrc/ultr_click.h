// ultr_click.h - the simulated user: one view of a click model (ClickModel: the two tables, their sizes, PBM / cascade / UBM / trust), the one
// statement of when it is valid (click_model_ok), the per-position decisions (click_decide) and the walk of one wavefront over one
// list (wave_click_walk).  Every kernel that draws clicks goes through the walk: click_draw (ultr_feed.h), online_rerank_kernel
// (ultr_online.hip), dbgd_interleave_kernel (ultr_dbgd.hip) and prop_wave (ultr_propensity.hip); prop_packed, several lists per
// wavefront, keeps its own loop over click_decide's pieces.  What differs between them stays with them: where a label comes from, where
// a click goes, the counter words that name the list, and what is redrawn while a list has no click.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"

// exam: [n_exam] for PBM / cascade, the dense [n_exam][n_exam] image of the triangular rank x distance table for UBM, the dense
// [2][n_exam] image alpha | beta of the trust-bias model; cprob: [n_rel]
struct ClickModel {
  const float* exam;
  const float* cprob;
  int n_exam, n_rel, model;
};

// the model of an argument block (ultr_click_args, ultr_online_args, ultr_dbgd_args, ultr_propensity_args name the fields alike)
template <class A>
__host__ __device__ __forceinline__ ClickModel click_model_of(const A& a) {
  return ClickModel{a.exam_prob, a.click_prob, a.n_exam, a.n_rel, a.click_model};
}

// what every entry refuses with ULTR_E_BADARG (UBM's walk reads column n_exam - 2 of the last row)
inline bool click_model_ok(const ClickModel& m) {
  return m.exam && m.cprob && m.n_exam > 0 && m.n_rel > 0 &&
         (m.model == ULTR_CLICK_PBM || m.model == ULTR_CLICK_CASCADE || m.model == ULTR_CLICK_UBM || m.model == ULTR_CLICK_TRUST) &&
         !(m.model == ULTR_CLICK_UBM && m.n_exam < 2);
}

// click probability of a relevance label: cprob[min(max((int)y, 0), n_rel - 1)]
__device__ __forceinline__ float click_prob_of(const ClickModel& cm, float y) {
  const int lab = y > 0.f ? (int)y : 0;
  return cm.cprob[lab < cm.n_rel ? lab : cm.n_rel - 1];
}
// user-browsing examination probability of `rank` at distance dist = rank - last click (last click -1 before the first one) in the dense
// [n_exam][n_exam] image of the triangular table (row = rank, column = distance - 1); getExamProb, click_models.py:175-186: beyond the
// table the LAST row serves - the last entry when no click precedes the position, else column distance - 1 saturating at the
// second-to-last
__device__ __forceinline__ float ubm_exam_prob(const ClickModel& cm, int rank, int dist) {
  const float* exam = cm.exam;
  const int n_exam = cm.n_exam;
  if (rank < n_exam) return exam[rank * n_exam + dist - 1];
  if (dist > rank) return exam[(n_exam - 1) * n_exam + n_exam - 1];
  return exam[(n_exam - 1) * n_exam + (dist < n_exam - 1 ? dist - 1 : (n_exam >= 2 ? n_exam - 2 : 0))];
}

// Trust bias: P(click) = alpha_k cp + beta_k, the product and the sum each rounded on its own (contraction is off in this body: a fused
// multiply-add would round once, and numpy float32 could not restate the decision bit for bit)
__device__ __forceinline__ float trust_click_prob(float alpha, float cp, float beta) {
#pragma clang fp contract(off)
  const float prod = alpha * cp;
  return prod + beta;
}

// The click decision of position l = l0 + lane (in: l < L) of one chunk of 64 positions of an L-position list, from its label y and its
// uniform u: PBM, cascade, UBM or trust bias (no carried state, as PBM) as ultr_click_batch draws them.  clicked_before (cascade: a click in an earlier chunk) and last_click
// (UBM: the rank of the last click so far) are wave-uniform and carried from chunk to chunk; the caller starts them at false / -1.
// (The body takes the tables as __restrict__ parameters, the one place where the compiler honours the qualifier: the table reads do
// not alias the clicks the caller writes between two chunks.  Without it update_tiled_kernel, which carries click_draw as a rider,
// waits for memory in the update's own branch - profiles/click_sim.md.)
__device__ __forceinline__ float click_decide_tables(const float* __restrict__ exam, const float* __restrict__ cprob, int n_exam, int n_rel,
                                                     int model, int L, int l0, int lane, bool in, float y, float u, bool& clicked_before,
                                                     int& last_click) {
  const ClickModel cm{exam, cprob, n_exam, n_rel, model};
  const int l = l0 + lane;
  float ck = 0.f;
  if (in) {
    const float cp = click_prob_of(cm, y);
    if (cm.model == ULTR_CLICK_UBM) {
      // click iff u < exam x cp: the walk below compares u / cp with the examination probability; cp == 0 (a relevance level that
      // is never clicked) gives +inf or NaN, and both compare false against every probability - no click, as intended
      ck = u / cp;
    } else if (cm.model == ULTR_CLICK_TRUST) {
      const int k = l < cm.n_exam ? l : cm.n_exam - 1;
      ck = (u < trust_click_prob(cm.exam[k], cp, cm.exam[cm.n_exam + k])) ? 1.f : 0.f;
    } else {
      ck = (u < cm.exam[l < cm.n_exam ? l : cm.n_exam - 1] * cp) ? 1.f : 0.f;
    }
  }
  if (cm.model == ULTR_CLICK_UBM) {
    const float ratio = ck;
    ck = 0.f;
    const int hi = (L - l0) < 64 ? (L - l0) : 64;
    for (int k = 0; k < hi; ++k) {
      const int rank = l0 + k;
      const float ex = ubm_exam_prob(cm, rank, rank - last_click);
      const float rk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ratio), k));
      const bool hit = rk < ex;
      if (hit) last_click = rank;
      if (lane == k && hit) ck = 1.f;
    }
  }
  if (cm.model == ULTR_CLICK_CASCADE) {  // only the first click of the list counts (the draws behind it are made and ignored, as in the reference)
    const uint64_t hit = __ballot(ck > 0.f);
    const int first = hit ? (int)__builtin_ctzll(hit) : 64;
    if (clicked_before || lane > first) ck = 0.f;
    clicked_before = clicked_before || hit != 0;
  }
  return ck;
}
__device__ __forceinline__ float click_decide(const ClickModel& cm, int L, int l0, int lane, bool in, float y, float u,
                                              bool& clicked_before, int& last_click) {
  return click_decide_tables(cm.exam, cm.cprob, cm.n_exam, cm.n_rel, cm.model, L, l0, lane, in, y, u, clicked_before, last_click);
}

// One wavefront draws the clicks of one list of n positions, in chunks of 64: position l takes its label from label(l) and its uniform
// from word l % 4 of Philox(c0, c1, l / 4, tag), click_decide decides with the carried state started afresh, store(l, click) puts the
// click where the caller wants it.  Returns the number of clicks of the list (wave-uniform).
template <class Label, class Store>
__device__ __forceinline__ float wave_click_walk(const ClickModel& cm, const Philox& rng, uint32_t c0, uint32_t c1, uint32_t tag, int n,
                                                 int lane, Label label, Store store) {
  float any = 0.f;
  bool clicked_before = false;
  int last_click = -1;
  for (int l0 = 0; l0 < n; l0 += 64) {
    const int l = l0 + lane;
    const bool in = l < n;
    float y = 0.f, u = 0.f;
    if (in) {
      y = label(l);
      u = u01(philox_word(rng, c0, c1, l, tag));
    }
    const float ck = click_decide(cm, n, l0, lane, in, y, u, clicked_before, last_click);
    if (in) store(l, ck);
    any += ck;
  }
  return wave_sum(any);
}
