// ultr_rowgrad.hip - the row-gradient kernels of the staged models (DLCM, GSF) and their launchers: column sums per row chunk and
// weight gradients with the rows split over the grid.  No atomics: every partial is added by the backward's one fold launch, in a fixed
// order.  Declarations: ultr_rowgrad.h; the scheme: DESIGN.md section 3d.
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_rowgrad.h"

namespace {

// ---- column sums (bias gradients, d beta, d gamma = sum d u o xhat): every job of the table in one launch --------------------------------
// A workgroup owns 16 columns of RG_CS_ROWS rows: 16 groups of threads each add every 16th row in order (in double), fixed-order combine,
// one partial per row chunk.  LDS: 2 KiB.
__global__ __launch_bounds__(256) void rg_colsum_kernel(RgCsTable tb) {
  __shared__ double sm[16][16];
  int j = 0;
  while (j + 1 < tb.n && (int)blockIdx.x >= tb.job[j + 1].blk_begin) ++j;
  const RgCsJob jb = tb.job[j];
  const int blk = (int)blockIdx.x - jb.blk_begin, chunk = blk / jb.ncb;
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = (blk - chunk * jb.ncb) * 16 + cl;
  const int64_t t0 = (int64_t)chunk * RG_CS_ROWS, t1 = t0 + RG_CS_ROWS < jb.T ? t0 + RG_CS_ROWS : jb.T;
  double acc = 0.0;
  if (c < jb.W) {
    for (int64_t t = t0 + grp; t < t1; t += 16) {
      float v = jb.a[t * jb.W + c];
      if (jb.mul != nullptr) {
        float h = jb.mul[t * jb.W + c];
        if (jb.mean != nullptr) h = (h - jb.mean[t]) * jb.rstd[t];
        v *= h;
      }
      acc += (double)v;
    }
  }
  sm[grp][cl] = acc;
  __syncthreads();
  if (grp == 0 && c < jb.W) {
    double t = sm[0][cl];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += sm[g][cl];
    jb.part[(int64_t)chunk * jb.W + c] = (float)t;
  }
}

// ---- weight gradients over the rows: part[s][n][f] = sum over the rows t of split s of G[t][n] U[t][f] -----------------------------------
// A wave owns 16 rows x 64 columns of the weight and walks its split four rows of K per matrix-core step: lane (i, q) supplies
// G[t + q][n0 + i] and U[t + q][f0 + 16 c + i], 64-byte runs of both.  U = fmaf((x - mu) * rr, ga, be) with the row's mean and rstd
// (STATS; rstd NULL: 1, a wave-uniform test), or with mu = 0, rr = 1, where the same expression is X gamma + beta exactly.  MASK: rows
// with t % mask_L == mask_L - 1 do not count.  Both are compile-time: an instance carries neither loads nor a 64-bit remainder it does
// not need.  A masked-out row or column supplies 0.
template <bool STATS, bool MASK>
__global__ __launch_bounds__(256) void rg_wgrad_kernel(const float* __restrict__ G, int Rn, const float* __restrict__ X, int N, int64_t K,
                                                       int mask_L, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, int64_t chunk,
                                                       float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int n0 = ((int)blockIdx.x * 4 + wave) * 16, f0 = (int)blockIdx.y * 64;
  if (n0 >= Rn) return;
  const int64_t t_begin = (int64_t)blockIdx.z * chunk, t_end = t_begin + chunk < K ? t_begin + chunk : K;
  const bool nok = n0 + i < Rn, normed = rstd == nullptr;
  const Src gs = make_src(G, K * Rn), xs = make_src(X, K * N), ms = make_src(mean, STATS ? K : 0), rs = make_src(rstd, STATS ? K : 0);
  bool fok[4];
  float ga[4], be[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int f = f0 + 16 * c + i;
    fok[c] = f < N;
    ga[c] = (gamma != nullptr && fok[c]) ? gamma[f] : 1.0f;
    be[c] = (beta != nullptr && fok[c]) ? beta[f] : 0.0f;
  }
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int len = (int)(t_end - t_begin);  // (32 bits: rg_wgrad's precondition)
  for (int r0 = 0; r0 < len; r0 += 4) {
    const int64_t t = t_begin + r0 + q;
    const bool tok = t < t_end;
    const bool aok = tok && nok && (!MASK || (int)(t % mask_L) != mask_L - 1);
    const float a = buf_ld1(gs, aok ? (unsigned)((t * Rn + n0 + i) * 4) : ULTR_OOB);
    float mu = 0.0f, rr = 1.0f;
    if constexpr (STATS) {
      mu = buf_ld1(ms, tok ? (unsigned)(t * 4) : ULTR_OOB);
      rr = normed ? 1.0f : buf_ld1(rs, tok ? (unsigned)(t * 4) : ULTR_OOB);
    }
    float x[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = buf_ld1(xs, (tok && fok[c]) ? (unsigned)((t * N + f0 + 16 * c + i) * 4) : ULTR_OOB);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = mfma16(a, (tok && fok[c]) ? fmaf((x[c] - mu) * rr, ga[c], be[c]) : 0.0f, acc[c]);
  }
  float* ps = part + (int64_t)blockIdx.z * Rn * N;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + 4 * q + r, col = f0 + 16 * c + i;
      if (row < Rn && col < N) ps[(int64_t)row * N + col] = acc[c][r];
    }
}

}  // namespace

int64_t RgCsTable::add(SrFoldQueue& folds, const float* a, const float* mul, const float* mean, const float* rstd, int64_t T, int W,
                       float* part, float* dst, hipStream_t st) {
  assert(n < RG_MAX_CS);
  const int chunks = (int)rg_cs_chunks(T);
  RgCsJob& j = job[n++];
  j.a = a; j.mul = mul; j.mean = mean; j.rstd = rstd; j.part = part; j.T = T; j.W = W; j.ncb = (W + 15) / 16; j.blk_begin = nblocks;
  nblocks += j.ncb * chunks;
  folds.add(part, (int64_t)W, chunks, W, dst, st, /*own_buffer=*/true);
  return (int64_t)chunks * W;
}

void RgCsTable::launch(hipStream_t st) const { hipLaunchKernelGGL(rg_colsum_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, *this); }

void rg_wgrad(SrFoldQueue& folds, const float* G, int Rn, const float* X, int N, int64_t K, int mask_L, const float* mean, const float* rstd,
              const float* gamma, const float* beta, float* part, float* dst, hipStream_t st) {
  if (K <= 0) {  // no row at all (DLCM's dW_hh at a single token: it has no previous state)
    (void)hipMemsetAsync(dst, 0, (size_t)Rn * N * sizeof(float), st);
    return;
  }
  const int64_t chunk = rg_wg_chunk(K);
  const int splits = (int)rg_wg_splits(K);
  const dim3 grid((unsigned)((Rn + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)splits);
  assert(K < ((int64_t)1 << 29) && !(mean != nullptr && mask_L != 0));  // (statistics with a mask: no model needs the instance yet)
  const auto kern = mean != nullptr ? rg_wgrad_kernel<true, false> : mask_L != 0 ? rg_wgrad_kernel<false, true> : rg_wgrad_kernel<false, false>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, G, Rn, X, N, K, mask_L, mean, rstd, gamma, beta, chunk, part);
  folds.add(part, (int64_t)Rn * N, splits, Rn * N, dst, st, /*own_buffer=*/true);
}

void rg_fold_all(SrFoldQueue& folds, const void* loss_ws, int n_loss_parts, int list_size, float* tail_dst, hipStream_t st) {
  if (loss_ws != nullptr && n_loss_parts > 0) {  // the step tail
    const int tail = (int)ultr_tail_len(list_size);
    folds.add((const float*)loss_ws, (int64_t)tail, n_loss_parts, tail, tail_dst, st, /*own_buffer=*/true);
  }
  folds.flush(st);
}
