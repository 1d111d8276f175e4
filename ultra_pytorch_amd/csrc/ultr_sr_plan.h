// ultr_sr_plan.h - what the host side of SetRank agrees on before a launch (host only: no kernel lives here): the parameter, saved-
// activation and workspace plan of a descriptor (SrPlan: sr_make_plan, and sr_make_score_plan for the forward no backward follows), the
// knobs, the context of ONE ultr_setrank_forward / _score / _backward call
// (SrCall) and the ROUTE of a step (SrRoute, sr_route): which launches its forward and its backward take, decided once per call from the
// same inputs on both sides.  Included by ultr_setrank.hip (the step), ultr_sr_rows.hip and ultr_sr_block.hip (the launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_sr_bwd.h"

#define SR_EPS 1e-6f  // nn.LayerNorm(eps=1e-6) everywhere in SetRank.py (:100-101, :134)
#define SR_ROWS 4     // rows per workgroup (= waves) of the row-wise kernels
#define SR_CS_ROWS 128  // rows per partial of the column-sum kernels
#define SR_LB_ROWS 64   // rows per workgroup (and per partial) of the fused LayerNorm backward

struct SrLayer {  // offsets (floats) into the flat parameter vector
  int64_t wd, bd, wf1, bf1, wf2, bf2, g1, b1, g2, b2;
};
struct SrPlan {
  int F, d, H, nl, dff, dh;
  int att_f16;  // 1: fp16-operand attention kernels (ultr_setrank_desc::attention_dtype)
  int64_t T;
  int64_t g_in, b_in, w1, b1, w2, b2, wo1, bo1, wo2, bo2;
  SrLayer lay[8];
  int64_t P;
  // saved activations (floats)
  int64_t sv_xg, sv_mean_in, sv_rstd_in, sv_xn0, sv_h0, sv_oh;
  int64_t sv_x[9];  // x_0 .. x_nl  [T, d]
  int64_t sv_A[8], sv_s1[8], sv_m1[8], sv_r1[8], sv_out1[8], sv_f[8], sv_s2[8], sv_m2[8], sv_r2[8];
  int64_t sv_lse[8];  // [T, H] attention row statistic (log-sum-exp of the scaled scores)
  int64_t sv_total;
  // split-half weight planes (round 4; ultr_gemm.h run_h3): behind the saved activations, rebuilt by every forward - for every
  // weight matrix W[M][K] with M >= 16 the planes hi | lo of 2^8 W as [M][ldK] halves (forward: Y = X W^T) and of W^T as [K][ldM]
  // halves (dgrad: dX = dY W), ldK / ldM = K / M rounded up to 32, zero-padded.  Offsets in HALVES from sv_planes (a float offset).
  int64_t sv_planes, planes_halves;
  int64_t sv_flag;   // float offset in `saved` of the range word behind the planes (ULTR_H3_FLAG_*: raised by sr_split_planes_kernel)
  int no_h3;         // ultr_setrank_desc::flags & ULTR_MODEL_FP32_PRODUCTS
  int stream_bwd;    // ultr_setrank_desc::flags & ULTR_MODEL_SR_STREAM_BWD: the streaming attention backward where the one-pass kernels refuse
  struct SplitMat { int64_t off; int M, K, ldK, ldM; int64_t f_off, t_off, g_off, gt_off; };  // g_off: fragment-major forward copy (sr_block_fwd_kernel), -1: none
                                                                                            // gt_off: fragment-major copy of W^T (out K, contraction M: the dgrad
                                                                                            // products of ultr_sr_bwd.hip), -1: none
  int n_split;
  SplitMat split[32];
  // workspace (floats)
  int maxw;
  int64_t ws_g[3];   // three [T, maxw] gradient buffers
  int64_t ws_part;   // [n_cs][3 * maxw] column-sum partials
  int n_cs, n_lb;
  int64_t ws_wg;     // [wg_split][max M*K] partial weight gradients (split over lists: one launch would run a
                     // [M, K] = dY^T X product with T = 100k contraction rows on a handful of workgroups)
  int wg_split;      // chunks of whole lists, divides the batch
  int64_t wg_floats; // floats of one weight-gradient partial region
  // the backward queues every partial-sum fold and runs them as ONE launch at its end (sr_fold_all_kernel): partials then
  // cannot share scratch, each producer takes a fresh piece of this arena
  int64_t ws_arena, arena_floats;
  int64_t ws_attn_t; // [T, H] t = dA . A of the streaming attention backward (stream_bwd only: other descriptors keep their size); else -1
  int64_t ws_total;
  int bwd_fused;     // the widths ultr_sr_bwd.hip takes: transposed fragment copies exist, the arena holds its per-workgroup partials
  int score;         // 1: the scoring plan (sr_make_score_plan) - no backward follows; sv_* offsets < 0 are rows nobody stores, the others alias
                     // a few buffers, and the fused launches keep every row but x_{l+1} on chip
};

// row chunks of sr_wgrad_kernel for an [M, K] gradient: about two workgroups per CU, chunks of a multiple of 32 rows
// (4 waves x 8 rows per trip), at most 128 of them
inline int sr_wgrad_chunks(int64_t T, int M, int K, int* rows_per_chunk) {
  const int tiles = ((M + 63) / 64) * ((K + 63) / 64);
  int S = (512 + tiles - 1) / tiles;
  if (S > 128) S = 128;
  int64_t rps = (T + S - 1) / S;
  rps = (rps + 31) / 32 * 32;
  if (rps < 32) rps = 32;
  *rows_per_chunk = (int)rps;
  return (int)((T + rps - 1) / rps);
}

// score: the activation layout of ultr_setrank_score (below) instead of the backward's complete record
inline bool sr_make_plan_any(const ultr_setrank_desc* c, int64_t T, SrPlan* p, bool score) {
  if (!c || c->feature_size <= 0 || c->d_model <= 0 || c->num_heads <= 0 || c->num_layers <= 0 || c->num_layers > 8 ||
      c->dff <= 0 || c->d_model % c->num_heads != 0 || (c->attention_dtype != ULTR_ATTN_FP32 && c->attention_dtype != ULTR_ATTN_FP16))
    return false;
  memset(p, 0, sizeof(*p));
  p->F = c->feature_size; p->d = c->d_model; p->H = c->num_heads; p->nl = c->num_layers; p->dff = c->dff;
  p->dh = p->d / p->H;
  p->att_f16 = (c->attention_dtype == ULTR_ATTN_FP16) ? 1 : 0;
  p->no_h3 = (c->flags & ULTR_MODEL_FP32_PRODUCTS) ? 1 : 0;
  p->stream_bwd = (c->flags & ULTR_MODEL_SR_STREAM_BWD) ? 1 : 0;
  p->T = T;
  p->score = score ? 1 : 0;
  const int64_t F = p->F, d = p->d, dff = p->dff;
  // THE parameter layout: every tensor starts where the one before it ends, in the reference's state_dict order
  //   g_in | b_in | W1 | b1 | W2 | b2 | Wo1 | bo1 | wo2 | bo2 | per layer: Wd | bd | Wf1 | bf1 | Wf2 | bf2 | g1 | b1 | g2 | b2
  // (each line below is `x = o; o += size of x`, so the next offset IS x + size: nothing in between, nothing reordered).  The fused launches
  // and the fold queue rely on it without asking again - a slab or a per-workgroup partial laid out as a run of neighbours
  // (W | b;  g | b;  Wo1 | bo1 | wo2 | bo2;  g_in .. b2) folds into the gradient vector as ONE job.
  int64_t o = 0;
  p->g_in = o; o += F;  p->b_in = o; o += F;
  p->w1 = o; o += dff * F;  p->b1 = o; o += dff;
  p->w2 = o; o += d * dff;  p->b2 = o; o += d;
  p->wo1 = o; o += dff * d; p->bo1 = o; o += dff;
  p->wo2 = o; o += dff;     p->bo2 = o; o += 1;
  for (int l = 0; l < p->nl; ++l) {
    SrLayer& y = p->lay[l];
    y.wd = o; o += d * d;    y.bd = o; o += d;
    y.wf1 = o; o += dff * d; y.bf1 = o; o += dff;
    y.wf2 = o; o += d * dff; y.bf2 = o; o += d;
    y.g1 = o; o += d; y.b1 = o; o += d;
    y.g2 = o; o += d; y.b2 = o; o += d;
  }
  p->P = o;
  int64_t s = 0;
  auto take = [&](int64_t n) { const int64_t at = s; s += (n + 3) & ~(int64_t)3; return at; };
  if (!score) {
    p->sv_xg = take(T * F); p->sv_mean_in = take(T); p->sv_rstd_in = take(T); p->sv_xn0 = take(T * F);
    p->sv_h0 = take(T * dff);
    for (int l = 0; l <= p->nl; ++l) p->sv_x[l] = take(T * d);
    for (int l = 0; l < p->nl; ++l) {
      p->sv_A[l] = take(T * d); p->sv_s1[l] = take(T * d); p->sv_m1[l] = take(T); p->sv_r1[l] = take(T);
      p->sv_out1[l] = take(T * d); p->sv_f[l] = take(T * dff);
      p->sv_s2[l] = take(T * d); p->sv_m2[l] = take(T); p->sv_r2[l] = take(T);
      p->sv_lse[l] = take(T * p->H);
    }
    p->sv_oh = take(T * dff);
  } else {
    // The scoring layout: what a forward without a backward keeps alive, F + dff + 4 d floats per token whatever the depth -
    //   X0 | X1  [T, d]    x_l and x_{l+1} ping-pong (a block reads one and writes the other)
    //   A        [T, d]    the attention's output
    //   S        [T, d]    separate launches: the pre-norm sum s1, then out1 = LN1(s1) IN PLACE (a row kernel: a lane reads its columns of
    //                      its row before it writes them); s2 lands in x_{l+1}'s buffer and LN2 runs in place there
    //   Hd       [T, dff]  separate launches: h0, every f_l, oh in turn
    //   Xn       [T, F]    separate launches: the normalised input rows (the gathered rows are not kept)
    // Statistics rows and lse: -1 everywhere.  On the fused launches S, Hd and Xn stay unused (the rows live in LDS): the launchers
    // pass -1 for them (p.score).  The plan is a function of the descriptor and T alone, so it holds the separate route's buffers always.
    const int64_t X0 = take(T * d), X1 = take(T * d), A = take(T * d), S = take(T * d), Hd = take(T * dff), Xn = take(T * F);
    p->sv_xg = p->sv_mean_in = p->sv_rstd_in = -1;
    p->sv_xn0 = Xn; p->sv_h0 = Hd; p->sv_oh = Hd;
    for (int l = 0; l <= p->nl; ++l) p->sv_x[l] = (l & 1) ? X1 : X0;
    for (int l = 0; l < p->nl; ++l) {
      p->sv_A[l] = A; p->sv_s1[l] = S; p->sv_out1[l] = S; p->sv_f[l] = Hd; p->sv_s2[l] = p->sv_x[l + 1];
      p->sv_m1[l] = p->sv_r1[l] = p->sv_m2[l] = p->sv_r2[l] = p->sv_lse[l] = -1;
    }
  }
  p->sv_total = s;
  {
    int64_t h = 0;
    auto add = [&](int64_t off, int64_t M, int64_t K) {
      SrPlan::SplitMat& m = p->split[p->n_split++];
      m.off = off; m.M = (int)M; m.K = (int)K;
      m.ldK = (int)((K + 31) / 32 * 32); m.ldM = (int)((M + 31) / 32 * 32);
      m.f_off = h; h += 2 * M * m.ldK;
      m.t_off = h; h += 2 * K * m.ldM;
      m.g_off = -1;
      m.gt_off = -1;
    };
    add(p->w1, dff, F); add(p->w2, d, dff); add(p->wo1, dff, d);
    for (int l = 0; l < p->nl; ++l) { add(p->lay[l].wd, d, d); add(p->lay[l].wf1, dff, d); add(p->lay[l].wf2, d, dff); }
    // fragment-major split-half copies (ultr_h3_index) of the encoder blocks' three matrices for the fused block kernel
    if (d % 32 == 0 && dff % 32 == 0)
      for (int k = 0; k < p->n_split; ++k) {  // (every matrix: the embedding FFN and the output FFN have fused kernels too)
        SrPlan::SplitMat& m = p->split[k];
        if (m.M % 32 != 0) continue;
        h = (h + 7) & ~(int64_t)7;  // 16-byte aligned: the kernel streams it with 16-byte buffer loads
        m.g_off = h;
        h += 2 * (int64_t)m.M * m.ldK;
      }
    // ... and of the transposes of the encoder blocks' matrices for the fused backward launches (ultr_sr_bwd.hip)
    p->bwd_fused = (d == SR_BWD_D && dff == SR_BWD_DFF) ? 1 : 0;
    if (p->bwd_fused)
      for (int k = 0; k < p->n_split; ++k) {  // (every matrix: the output FFN and the embedding FFN have fused backward launches too)
        SrPlan::SplitMat& m = p->split[k];
        h = (h + 7) & ~(int64_t)7;
        m.gt_off = h;
        h += 2 * (int64_t)((m.K + 31) / 32 * 32) * m.ldM;  // whole 32-column chunks (a ragged last chunk keeps its tail unwritten: those
                                                           // output columns do not exist)
      }
    p->sv_planes = (p->sv_total + 4 + 7) & ~(int64_t)7;
    p->planes_halves = h;
    p->sv_flag = p->sv_planes + (h + 1) / 2;  // (ultr_setrank_saved_bytes leaves four floats behind the planes)
  }
  p->maxw = (int)(F > d ? F : d);
  if (dff > p->maxw) p->maxw = (int)dff;
  int64_t w = 0;
  for (int k = 0; k < 3; ++k) { p->ws_g[k] = w; w += (T * p->maxw + 3) & ~(int64_t)3; }
  p->n_cs = (int)((T + SR_CS_ROWS - 1) / SR_CS_ROWS);
  p->n_lb = (int)((T + SR_LB_ROWS - 1) / SR_LB_ROWS);
  p->ws_part = w; w += (int64_t)p->n_lb * 3 * p->maxw;  // n_lb >= n_cs
  // sum-of-squares partials for ultr_apply_update live at offset 0 of a SEPARATE region at the end (ultr_grad_sumsq
  // writes them at the start of the pointer it is given)
  // weight-gradient split: the largest divisor of T that leaves chunks of >= 512 rows, at most 128 chunks
  p->wg_split = 1;
  for (int sdiv = 2; sdiv <= 128 && T / sdiv >= 512; ++sdiv)
    if (T % sdiv == 0) p->wg_split = sdiv;
  int64_t maxmk = dff * F;
  if (d * dff > maxmk) maxmk = d * dff;
  if (d * d > maxmk) maxmk = d * d;
  int64_t wg_floats = (int64_t)p->wg_split * maxmk;  // the plain chunked kernel (unaligned shapes)
  const int shapes[4][2] = {{(int)dff, (int)F}, {(int)d, (int)dff}, {(int)d, (int)d}, {(int)dff, (int)d}};  // [M, K]
  for (int k = 0; k < 4; ++k) {
    int rps = 0;
    const int64_t need = (int64_t)sr_wgrad_chunks(T, shapes[k][0], shapes[k][1], &rps) * ((int64_t)shapes[k][0] * shapes[k][1] + shapes[k][0]);
    if (need > wg_floats) wg_floats = need;
  }
  p->ws_wg = w; w += wg_floats;
  p->wg_floats = wg_floats;
  p->arena_floats = (int64_t)(3 * p->nl + 4) * ((wg_floats + 3) & ~(int64_t)3) + (int64_t)(2 * p->nl + 5) * p->n_lb * 3 * p->maxw;
  if (p->bwd_fused)  // two per block, the output FFN's, the embedding FFN's
    p->arena_floats += (int64_t)(2 * p->nl + 1) * SR_BWD_MAXWG * (d * dff + dff + 3 * d + 4) + (int64_t)SR_BWD_MAXWG * (2 * F + dff * F + dff + d * dff + d + 4);
  w = (w + 3) & ~(int64_t)3;  // 16-byte pieces (the vector form of sr_fold_all_kernel)
  p->ws_arena = w; w += p->arena_floats;
  p->ws_attn_t = -1;
  if (p->stream_bwd) {
    w = (w + 3) & ~(int64_t)3;
    p->ws_attn_t = w; w += (T * p->H + 3) & ~(int64_t)3;
  }
  p->ws_total = w;
  return true;
}
// the plan of ultr_setrank_forward / _backward: `saved` is the backward's complete record
inline bool sr_make_plan(const ultr_setrank_desc* c, int64_t T, SrPlan* p) { return sr_make_plan_any(c, T, p, false); }
// the plan of ultr_setrank_score: same parameters, planes and range word, the activations of the scoring layout.  setrank_forward runs
// against either plan; the workspace fields (the backward's) mean nothing here.
inline bool sr_make_score_plan(const ultr_setrank_desc* c, int64_t T, SrPlan* p) { return sr_make_plan_any(c, T, p, true); }

// Knobs of SetRank (README.md): read from the environment ONCE (first use), replaced whole by ultr_config_reload(); every call
// takes one copy into its context, so one forward or backward sees one set of values.  Storage and loader: ultr_setrank.hip.
struct SrKnobs {
  bool loaded;
  int h3;         // ULTR_SR_H3 (default 1): the Linear products on split-half planes of the weights (fp16 matrix cores); 0: fp32 matrix cores
  int attn_h3;    // ULTR_SR_ATTN_H3 0: fp32 matrix cores; 1 (default): split-half BACKWARD kernel (the forward always runs on the fp32 matrix cores)
  int attn_mask;  // ULTR_SR_ATTN_H3_MASK (default -1 = all), debug: bit (2 layer + dir), dir 0 forward / 1 backward
  int wg_h3;      // ULTR_SR_WG_H3 (default 1): square-ish weight gradients on the DNN's split-half weight-gradient kernel
  int bwd_fused;  // ULTR_SR_BWD_FUSED bits (default 7 = all): 1 the row-local chain of a block's backward as two launches (ultr_sr_bwd.hip)
                  // instead of seven, 2 the output FFN's backward as one instead of three, 4 the embedding FFN's
  int attn_long_min;  // ULTR_SR_ATTN_LONG_MIN (default 257): the forward's attention streams its keys (ultr_sr_attn_long.hip) from this list size on;
                      // tests and measurement only - it lowers the hand-over point, beyond 256 documents the keys are streamed whatever it says
  int block;      // ULTR_SR_BLOCK 0: separate launches; 2: the round-5 kernels (two 8-wave workgroups per CU) everywhere; 3 (default): the persistent
                  // kernel of round 6 where its widths apply, 2 elsewhere.  (1, once a 16-wave form of the round-5 kernel, is read as 2.)
};
#define SR_CHECK(call)        \
  do {                        \
    const int rc_ = (call);   \
    if (rc_ != 0) return rc_; \
  } while (0)

// What ONE ultr_setrank_forward / _backward call hands to its helpers, built on that call's stack: the helpers read no global.
struct SrFoldQueue;  // ultr_sr_rows.h
struct SrCall {
  const SrPlan& p;
  const float* params;
  const _Float16* planes;  // split-half planes in `saved` (built by the forward); NULL: those products are off for this call (ULTR_SR_H3=0, ULTR_MODEL_FP32_PRODUCTS)
  SrKnobs knobs;
  int cus;
  float* sv;               // `saved` (the backward only reads it)
  float* ws;               // the backward's workspace, NULL in the forward
  hipStream_t st;
  SrFoldQueue* folds;      // the backward's, NULL in the forward
  // the planes of the weight matrix W[M][K] at float offset `off` of the parameter vector, NULL: none (the product runs in fp32)
  const SrPlan::SplitMat* split(int64_t off, int M, int K) const {
    if (planes == nullptr) return nullptr;
    for (int k = 0; k < p.n_split; ++k) {
      const SrPlan::SplitMat& m = p.split[k];
      if (m.off == off && m.M == M && m.K == K) return &m;
    }
    return nullptr;
  }
};

// ---- the route of a step ------------------------------------------------------------------------------------------------------------
// Which launches ONE step takes.  ultr_setrank_forward and ultr_setrank_backward each fill it once, before their first launch, from the
// same inputs (plan, knobs, split-half planes on or off, dropout step or not, `saved` 16-byte aligned or not - the planes sit a multiple of
// 16 bytes into `saved`), so the two sides of a step cannot disagree: the forward leaves out1 unwritten (skip_out1) exactly when the
// backward recomputes it.  What the route cannot see is a knob reload BETWEEN the two calls of a step: the caller must not do that, as it
// must not for the planes (built by the forward under ITS ULTR_SR_H3).
enum { SR_BLOCK_SEPARATE = 0, SR_BLOCK_ROUND5 = 1, SR_BLOCK_PERSISTENT = 2 };
struct SrRoute {
  // forward
  int embed;       // 1: gather + input LayerNorm + embedding FFN as one launch (sr_embed_fwd_kernel) - where the features pointer allows it,
                   // which only the forward holds: ultr_setrank_forward tests it at the launch
  int block;       // everything of an encoder block behind the attention: SR_BLOCK_SEPARATE (GEMM and LayerNorm launches), _ROUND5
                   // (sr_block_fwd_kernel), _PERSISTENT (sr_fwd_block_kernel)
  int head_rides;  // the output FFN runs inside the last block's launch
  int skip_out1;   // the forward runs a block kernel AND the backward runs the blocks fused: out1 is neither written nor read
  // backward: the fused launches of ultr_sr_bwd.hip
  int bwd_head, bwd_blocks, bwd_embed;
  // geometry
  int R, tiles, nwg;     // the persistent launches (both directions): rows per tile, tiles, workgroups
  int block_R, embed_R;  // the round-5 kernels: rows per workgroup
};
// rows per workgroup of a round-5 kernel: whole rounds of two 8-wave workgroups per CU, as many rows as their 80 KB of LDS hold (<= 32);
// 0: fewer than 16 fit
inline int sr_round5_rows(int64_t T, int cus, int64_t row_bytes, int64_t fixed_bytes) {
  int64_t rmax = (80 * 1024 - fixed_bytes) / row_bytes - 1;
  if (rmax > 32) rmax = 32;
  if (rmax < 16) return 0;
  const int64_t slots = (int64_t)cus * 2;
  const int64_t rounds = (T + slots * rmax - 1) / (slots * rmax);
  const int64_t R = (T + slots * rounds - 1) / (slots * rounds);
  return (int)(R < 16 ? 16 : R);
}
inline SrRoute sr_route(const SrPlan& p, const SrKnobs& k, int cus, bool planes_on, bool drop, bool aligned) {
  SrRoute r;
  memset(&r, 0, sizeof(r));
  if (drop || !planes_on) return r;  // a dropout step and the fp32 products run the separate launches throughout
  const int F = p.F, d = p.d, dff = p.dff;
  // The persistent launches: the plan's widths (p.bwd_fused: d 256, dff 64 - transposed fragment copies, arena pieces) and a row count
  // sr_bwd_geometry takes (it bounds T * d * 4 below 2^31 itself).  Its yes / no depends on T alone; the CU count only shapes R, tiles
  // and workgroups - so the two calls of a step agree on every field above the geometry whatever the device reports.
  const bool persistent = p.bwd_fused && sr_bwd_geometry(p.T, cus, &r.R, &r.tiles, &r.nwg);
  // The round-5 kernels: widths that are multiples of 32 (sr_make_plan then built the fragment-major copies of every matrix they read),
  // d <= 256, dff 32 / 64 / 128; the embedding kernel also wants whole float4s of at most 256 features.
  if (k.block != 0 && aligned && d % 32 == 0 && d >= 32 && d <= 256 && (dff == 32 || dff == 64 || dff == 128)) {
    r.block_R = sr_round5_rows(p.T, cus, (int64_t)(2 * (d + 8) + (dff + 8)) * 4, (int64_t)(6 * d + 3 * dff + 4 + 128) * 4);
    r.block = (k.block >= 3 && persistent) ? SR_BLOCK_PERSISTENT : r.block_R ? SR_BLOCK_ROUND5 : SR_BLOCK_SEPARATE;
    if (F % 4 == 0 && F <= 256) {
      r.embed_R = sr_round5_rows(p.T, cus, (int64_t)(((F + 31) / 32 * 32 + 8) + (dff + 8)) * 4, (int64_t)(2 * F + dff + d + 128) * 4);
      r.embed = r.embed_R != 0;
    }
  }
  r.head_rides = r.block != SR_BLOCK_SEPARATE;
  r.bwd_blocks = persistent && (k.bwd_fused & 1);
  r.bwd_head = persistent && (k.bwd_fused & 2);
  r.bwd_embed = persistent && (k.bwd_fused & 4) && F % 4 == 0 && F <= SR_BWD_D;
  r.skip_out1 = r.block != SR_BLOCK_SEPARATE && r.bwd_blocks;
  return r;
}

// the route's fused forward launches (ultr_sr_block.hip): encoder block l behind the attention as ONE launch (rt.block _ROUND5 or
// _PERSISTENT; with rt.head_rides the last block's launch also runs the output FFN), and the input side as one launch (rt.embed)
int sr_block_fwd(const SrCall& c, const SrRoute& rt, int l, float* scores);
int sr_embed_fwd(const SrCall& c, const SrRoute& rt, const float* feats, const int32_t* docids, int64_t n_docs, int batch, int L);
