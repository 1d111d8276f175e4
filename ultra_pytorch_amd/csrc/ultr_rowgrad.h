// ultr_rowgrad.h - the gradients a staged model's backward sums over its rows (kernels in ultr_rowgrad.hip): column sums per row chunk
// (bias, beta and gamma gradients) and weight gradients with the rows split over the grid.  Both leave partials that the backward's ONE
// fold launch adds in a fixed order (SrFoldQueue).  Called from ultr_dlcm.hip and ultr_gsf.hip; DESIGN.md section 3d.
#pragma once
#include "ultr_rowgrad_plan.h"
#include "ultr_sr_rows.h"

// ---- column sums: the jobs of one launch -----------------------------------------------------------------------------------
#define RG_MAX_CS 6
struct RgCsJob {
  const float* a;     // [T][W]
  const float* mul;   // NULL, or the same shape as a: sums of a o mul ...
  const float* mean;  // ... NULL, or with mean / rstd [T]: sums of a o ((mul - mean[t]) rstd[t])
  const float* rstd;
  float* part;        // [chunks][W]
  int64_t T;
  int W, ncb, blk_begin;
};
struct RgCsTable {
  int n = 0, nblocks = 0;
  RgCsJob job[RG_MAX_CS];  // (never zeroed: rg_colsum_kernel reads job[0 .. n) only)
  // queues the job and the fold of its partials into dst [W]; returns the floats of `part` it took
  int64_t add(SrFoldQueue& folds, const float* a, const float* mul, const float* mean, const float* rstd, int64_t T, int W, float* part,
              float* dst, hipStream_t st);
  void launch(hipStream_t st) const;
};

// ---- weight gradient: dst [Rn][N] = sum over the rows t < K of G[t][n] U[t][f] ------------------------------------------------
// G [K][Rn], X [K][N]; U = (X - mean[t]) rstd[t] gamma + beta, formed as X is read (mean NULL: no statistics; with a mean, rstd NULL: 1;
// gamma NULL: U = X).  mask_L != 0: rows with t % mask_L == mask_L - 1 do not count - not together with statistics.  K <= 0: dst is
// zeroed.  part: rg_wg_splits(K) Rn N floats.  Requires K < 2^29 rows and both operands below 2 GiB (32-bit row counts and byte offsets).
void rg_wgrad(SrFoldQueue& folds, const float* G, int Rn, const float* X, int N, int64_t K, int mask_L, const float* mean, const float* rstd,
              const float* gamma, const float* beta, float* part, float* dst, hipStream_t st);

// the end of a backward: the loss partials of the step tail (when the call carries them) join the queue, ONE launch folds all of it
void rg_fold_all(SrFoldQueue& folds, const void* loss_ws, int n_loss_parts, int list_size, float* tail_dst, hipStream_t st);
