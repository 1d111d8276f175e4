// ultr_sr_rows.h - SetRank's row-wise launches (kernels in ultr_sr_rows.hip): LayerNorm forward / backward, column sums, the scorer's
// row kernels, and the backward's queue of deferred folds.  Called from ultr_setrank.hip's separate-launch paths.
#pragma once
#include "ultr_sr_plan.h"

// ---- deferred folds -------------------------------------------------------------------------------------------------------
// ultr_setrank_backward produces ~20 sets of partial sums (weight-gradient slabs per row chunk, LayerNorm / bias column
// partials per row block); their folds only feed the update at the very end.  Instead of one 7 us launch behind every
// producer (21 of the step's 69 launches, 0.15 ms) the backward queues them and ONE launch folds all - same arithmetic
// order per job as sr_fold_kernel / sr_fold16_kernel, so the gradients keep their bits.
#define SR_MAX_FOLDS 72
struct SrFoldJob {
  const float* part;
  float* dst;
  int64_t stride;
  int nparts, len, wide, blk_begin;  // wide: 16 columns per workgroup (many partials) instead of 64
};
struct SrFoldTable {
  int n, nblocks;
  SrFoldJob job[SR_MAX_FOLDS];
};
// The queue of ONE backward, on setrank_backward's stack: flush() launches what was queued (an early error return just drops it).
struct SrFoldQueue {
  float* arena;
  int64_t cap, used;
  SrFoldTable tab;  // (never zeroed: sr_fold_all_kernel reads job[0 .. n) only)
  SrFoldQueue(float* arena_, int64_t cap_) : arena(arena_), cap(cap_), used(0) { tab.n = 0; tab.nblocks = 0; }
  // scratch for one producer's partials: a fresh arena piece while there is room, the shared region otherwise
  float* scratch(float* shared_region, int64_t floats) {
    const int64_t need = (floats + 3) & ~(int64_t)3;
    if (used + need <= cap && tab.n + 2 <= SR_MAX_FOLDS) {
      float* at = arena + used;
      used += need;
      return at;
    }
    return shared_region;
  }
  // a piece of the arena or NULL (producers whose partials do not fit the shared region: the fused launches of ultr_sr_bwd.hip, whose
  // pieces sr_make_plan sized the arena for - NULL there is ULTR_E_WORKSPACE, never another path)
  float* piece(int64_t floats) {
    const int64_t need = (floats + 3) & ~(int64_t)3;
    if (!(used + need <= cap && tab.n + 4 <= SR_MAX_FOLDS)) return nullptr;
    float* at = arena + used;
    used += need;
    return at;
  }
  // queues the fold of partials that nobody overwrites before flush() (an arena piece, or the caller's own buffer); a partial in a
  // shared region, or one more than the table holds, is folded by a launch of its own right here
  void add(const float* part, int64_t stride, int nparts, int len, float* dst, hipStream_t st, bool own_buffer = false);
  void flush(hipStream_t st);
};

// input LayerNorm on the gathered feature rows: xg = features[ids] (PAD -> zero row), xn0 = LN_in(xg); float4 kernel when the rows allow it
void sr_ln_gather_fwd(const float* feats, const int32_t* docids, int64_t n_docs, int batch, int L, int64_t T, int W, const float* gamma,
                      const float* beta, float* xg, float* y, float* mean_out, float* rstd_out, hipStream_t st);
// residual LayerNorm forward: y = LN(a + (b + bias)); float4 kernel when the rows allow it
void sr_ln_residual_fwd(const float* a, const float* b, const float* bias, int64_t T, int W, const float* gamma, const float* beta,
                        float* sum_out, float* y, float* mean_out, float* rstd_out, int batch, int L, hipStream_t st);
// dx = LayerNorm backward of dy (any width: the rows only)
void sr_ln_bwd_rows(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma, int W, float* dx);
// dx = LayerNorm backward of dy; dst_gb = dgamma | dbeta; dst_bias = column sums of dx (may be NULL).  W <= 1024.
int sr_ln_bwd_cs(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma, int W,
                 float* dx, float* dst_gb, float* dst_bias);
// dst[0..W) = d gamma, dst[W..2W) = d beta
void sr_colsum_ln(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, int W, float* dst);
// dst[0..W) = column sums of a (mode 0) or of a o xhat (mode 1)
void sr_colsum(const SrCall& c, const float* a, const float* s, const float* mean, const float* rstd, int W, int mode, float* dst);
// the scorer (width-1 output, SetRank.py:136): y[t] = X[t] . w + bias[0];  its weight gradient dst[0..K) = sum_t dy[t] X[t][k]
void sr_rowdot(const float* X, const float* w, const float* bias, float* y, int64_t T, int K, hipStream_t st);
void sr_colsum_w(const SrCall& c, const float* dy, const float* X, int K, float* dst);
// the scorer's backward in one pass (K = dff <= 256): G = d oh [T, K] (ReLU mask fused), dst = d wo2 | d bo2
void sr_head_bwd(const SrCall& c, const float* dy, const float* oh, const float* w, int K, float* G, float* dst);
