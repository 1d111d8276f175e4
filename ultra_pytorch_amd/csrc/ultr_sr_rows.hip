// ultr_sr_rows.hip - SetRank's row-wise kernels (rounds 1 - 4) and their launchers: feature gather + LayerNorm, residual + LayerNorm
// (forward, and backward fused with the gamma / beta / bias column sums), column sums, the scorer's two width-1 products and its
// one-pass backward, and the fixed-order folds of every partial sum (the backward's SrFoldQueue: ONE launch at its end).
// One wavefront per row or a workgroup per block of rows; no atomics.  Declarations: ultr_sr_rows.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_sr_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// row-wise kernels: one wavefront per row, SR_ROWS rows per workgroup
// ---------------------------------------------------------------------------------------------------------
// y = LayerNorm(a [+ (b [+ bias])]) * gamma + beta; optionally stores the pre-norm sum and the statistics.
// (b + bias is the preceding Linear's output: its bias add rides along instead of costing a pass of its own.)
// a_gather: a is the feature matrix and rows are gathered through the doc ids (PAD -> zero row).
// In place (y == a or y == b, the scoring forward): a lane reads and writes columns lane + 64 k of its wave's row only, and in every
// pass reads a column before it writes it.
__global__ __launch_bounds__(SR_ROWS * 64) void sr_ln_fwd_kernel(const float* a /* may alias y */, const float* b /* may alias y */,
                                                                const float* __restrict__ bias /* added to b, may be NULL */,
                                                                const int32_t* __restrict__ docids, int64_t n_docs, int B,
                                                                int L, int64_t T, int W, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ sum_out,
                                                                float* y, float* __restrict__ mean_out,
                                                                float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_ROWS + wave;
  if (n >= T) return;
  const float* ra = a + n * W;
  if (docids != nullptr) {
    const int bb = (int)(n / L), ll = (int)(n % L);
    const int id = docids[(int64_t)ll * B + bb];
    ra = (id >= 0 && id < n_docs) ? a + (int64_t)id * W : nullptr;
  }
  if (W <= 64 * 16) {
    // the row lives in registers between the passes (one read of a and b)
    float v[16];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = lane + 64 * k;
      v[k] = 0.f;
      if (c < W) {
        v[k] = ra ? ra[c] : 0.f;
        if (b != nullptr) v[k] += (bias != nullptr) ? b[n * W + c] + bias[c] : b[n * W + c];
        if (sum_out != nullptr) sum_out[n * W + c] = v[k];
      }
      s += v[k];
    }
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float dlt = (lane + 64 * k < W) ? v[k] - mean : 0.f;
      q += dlt * dlt;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + SR_EPS);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = lane + 64 * k;
      if (c < W) y[n * W + c] = (v[k] - mean) * rstd * gamma[c] + beta[c];
    }
    if (lane == 0) {
      if (mean_out) mean_out[n] = mean;
      if (rstd_out) rstd_out[n] = rstd;
    }
    return;
  }
  float s = 0.f;
  for (int c = lane; c < W; c += 64) {
    float v = ra ? ra[c] : 0.f;
    if (b != nullptr) v += (bias != nullptr) ? b[n * W + c] + bias[c] : b[n * W + c];
    if (sum_out != nullptr) sum_out[n * W + c] = v;
    s += v;
  }
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
  for (int c = lane; c < W; c += 64) {
    float v = ra ? ra[c] : 0.f;
    if (b != nullptr) v += (bias != nullptr) ? b[n * W + c] + bias[c] : b[n * W + c];
    const float dlt = v - mean;
    q += dlt * dlt;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + SR_EPS);
  for (int c = lane; c < W; c += 64) {
    float v = ra ? ra[c] : 0.f;
    if (b != nullptr) v += (bias != nullptr) ? b[n * W + c] + bias[c] : b[n * W + c];
    y[n * W + c] = (v - mean) * rstd * gamma[c] + beta[c];
  }
  if (lane == 0) {
    if (mean_out) mean_out[n] = mean;
    if (rstd_out) rstd_out[n] = rstd;
  }
}

// the input LayerNorm on gathered feature rows with 16-byte accesses (W % 4 == 0, W <= 1024): lane owns the float4
// chunks lane, lane + 64, ... of the row; stores the gathered row (for the backward; sum_out may be NULL) and the normalised row
__global__ __launch_bounds__(SR_ROWS * 64) void sr_ln_gather_v4_kernel(const float* __restrict__ feats, const int32_t* __restrict__ docids,
                                                                      int64_t n_docs, int B, int L, int64_t T, int W,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float* __restrict__ sum_out, float* __restrict__ y,
                                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_ROWS + wave;
  if (n >= T) return;
  const int bb = (int)(n / L), ll = (int)(n % L);
  const int id = docids[(int64_t)ll * B + bb];
  const float* ra = (id >= 0 && id < n_docs) ? feats + (int64_t)id * W : nullptr;  // PAD -> zero row
  const int nq = W / 4;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qd = lane + 64 * k;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (qd < nq) {
      if (ra != nullptr) v[k] = ld4(ra + 4 * qd);
      if (sum_out != nullptr) st4(sum_out + n * W + 4 * qd, v[k]);  // (NULL, wave-uniform: a scoring forward keeps no gathered rows)
    }
    s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (lane + 64 * k < nq) {
      const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + SR_EPS);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qd = lane + 64 * k, c = 4 * qd;
    if (qd < nq)
      st4(y + n * W + c, make_float4((v[k].x - mean) * rstd * gamma[c] + beta[c], (v[k].y - mean) * rstd * gamma[c + 1] + beta[c + 1],
                                     (v[k].z - mean) * rstd * gamma[c + 2] + beta[c + 2], (v[k].w - mean) * rstd * gamma[c + 3] + beta[c + 3]));
  }
  if (lane == 0 && mean_out != nullptr) {  // (both or neither: a scoring forward keeps no statistics)
    mean_out[n] = mean;
    rstd_out[n] = rstd;
  }
}

// the residual LayerNorms (W = d_model a multiple of 256, no gather): 16-byte accesses, NV float4 per lane
// In place (y == a or y == b): the whole row sits in registers before the first store to y.
template <int NV>
__global__ __launch_bounds__(SR_ROWS * 64) void sr_ln_fwd_v4_kernel(const float* a /* may alias y */, const float* b /* may alias y */,
                                                                   const float* __restrict__ bias, int64_t T,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ sum_out, float* y,
                                                                   float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  constexpr int W = NV * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_ROWS + wave;
  if (n >= T) return;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    const float4 av = ld4(a + n * W + c);
    if (b != nullptr) {  // wave-uniform: b == NULL = `a` already is the pre-norm sum (a GEMM epilogue wrote it)
      float4 bv = ld4(b + n * W + c);
      if (bias != nullptr) {
        bv.x += bias[c]; bv.y += bias[c + 1]; bv.z += bias[c + 2]; bv.w += bias[c + 3];  // parameters: any float offset
      }
      v[k] = make_float4(av.x + bv.x, av.y + bv.y, av.z + bv.z, av.w + bv.w);
      if (sum_out != nullptr) st4(sum_out + n * W + c, v[k]);
    } else {
      v[k] = av;
    }
    s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + SR_EPS);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    st4(y + n * W + c, make_float4((v[k].x - mean) * rstd * gamma[c] + beta[c], (v[k].y - mean) * rstd * gamma[c + 1] + beta[c + 1],
                                   (v[k].z - mean) * rstd * gamma[c + 2] + beta[c + 2], (v[k].w - mean) * rstd * gamma[c + 3] + beta[c + 3]));
  }
  if (lane == 0 && mean_out != nullptr) {  // (both or neither: a scoring forward keeps no statistics)
    mean_out[n] = mean;
    rstd_out[n] = rstd;
  }
}

// LayerNorm backward per row: ds = rstd * (g - mean(g) - xh * mean(g * xh)), g = dy * gamma, xh = (s - mean) * rstd.
// ds_out may be NULL (only the parameter gradients are wanted); accumulate: ds_out += instead of =.
__global__ __launch_bounds__(SR_ROWS * 64) void sr_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, int64_t T, int W,
                                                                float* __restrict__ ds_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_ROWS + wave;
  if (n >= T || ds_out == nullptr) return;
  const float m = mean[n], r = rstd[n];
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < W; c += 64) {
    const float g = dy[n * W + c] * gamma[c];
    const float xh = (s[n * W + c] - m) * r;
    s1 += g;
    s2 += g * xh;
  }
  s1 = wave_sum(s1) / (float)W;
  s2 = wave_sum(s2) / (float)W;
  for (int c = lane; c < W; c += 64) {
    const float g = dy[n * W + c] * gamma[c];
    const float xh = (s[n * W + c] - m) * r;
    ds_out[n * W + c] = r * (g - s1 - xh * s2);
  }
}

// LayerNorm backward AND every column sum that hangs off it, one pass over dy and s:
//   ds = the row gradient above;  part[blk][0:W] = sum_r dy xhat (dgamma),  [W:2W] = sum_r dy (dbeta),
//   [2W:3W] = sum_r ds (the bias gradient of the Linear that produced s).
// A workgroup owns SR_LB_ROWS rows, a wave every 4th of them (row in registers, KMAX columns per lane); the four
// waves' column partials are folded in fixed order through LDS.
template <int KMAX>
__global__ __launch_bounds__(256) void sr_ln_bwd_cs_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, int64_t T, int W,
                                                           float* __restrict__ ds_out, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4 waves][3][W]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SR_LB_ROWS;
  const int64_t r1 = (r0 + SR_LB_ROWS < T) ? r0 + SR_LB_ROWS : T;
  float gm[KMAX], ag[KMAX], ab[KMAX], ad[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int c = lane + 64 * k;
    gm[k] = (c < W) ? gamma[c] : 0.f;
    ag[k] = ab[k] = ad[k] = 0.f;
  }
  const float invw = 1.0f / (float)W;
  for (int64_t n = r0 + wave; n < r1; n += 4) {
    const float m = mean[n], r = rstd[n];
    float g[KMAX], xh[KMAX];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = lane + 64 * k;
      const float d = (c < W) ? dy[n * W + c] : 0.f;
      xh[k] = (c < W) ? (s[n * W + c] - m) * r : 0.f;
      g[k] = d * gm[k];
      s1 += g[k];
      s2 += g[k] * xh[k];
      ag[k] += d * xh[k];
      ab[k] += d;
    }
    s1 = wave_sum(s1) * invw;
    s2 = wave_sum(s2) * invw;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = lane + 64 * k;
      const float v = r * (g[k] - s1 - xh[k] * s2);
      if (c < W) {
        ds_out[n * W + c] = v;
        ad[k] += v;
      }
    }
  }
  float* mine = smem + (size_t)wave * 3 * W;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int c = lane + 64 * k;
    if (c < W) {
      mine[c] = ag[k];
      mine[W + c] = ab[k];
      mine[2 * W + c] = ad[k];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 3 * W; e += 256)
    part[(int64_t)blockIdx.x * 3 * W + e] = ((smem[e] + smem[3 * W + e]) + smem[6 * W + e]) + smem[9 * W + e];
}

// the same with 16-byte accesses (W a multiple of 256): lane owns columns 4 lane .. 4 lane + 3 (+ 256 k)
template <int NV>
__global__ __launch_bounds__(256) void sr_ln_bwd_cs_v4_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, int64_t T,
                                                              float* __restrict__ ds_out, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4 waves][3][W]
  constexpr int W = NV * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SR_LB_ROWS;
  const int64_t r1 = (r0 + SR_LB_ROWS < T) ? r0 + SR_LB_ROWS : T;
  float4 gm[NV], ag[NV], ab[NV], ad[NV];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    gm[k] = make_float4(gamma[c], gamma[c + 1], gamma[c + 2], gamma[c + 3]);  // parameters: any float offset
    ag[k] = ab[k] = ad[k] = z4;
  }
  const float invw = 1.0f / (float)W;
  for (int64_t n = r0 + wave; n < r1; n += 4) {
    const float m = mean[n], r = rstd[n];
    float4 g[NV], xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = 4 * lane + 256 * k;
      const float4 d = ld4(dy + n * W + c), sv = ld4(s + n * W + c);
      xh[k] = make_float4((sv.x - m) * r, (sv.y - m) * r, (sv.z - m) * r, (sv.w - m) * r);
      g[k] = make_float4(d.x * gm[k].x, d.y * gm[k].y, d.z * gm[k].z, d.w * gm[k].w);
      s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
      s2 += (g[k].x * xh[k].x + g[k].y * xh[k].y) + (g[k].z * xh[k].z + g[k].w * xh[k].w);
      ag[k].x += d.x * xh[k].x; ag[k].y += d.y * xh[k].y; ag[k].z += d.z * xh[k].z; ag[k].w += d.w * xh[k].w;
      ab[k].x += d.x; ab[k].y += d.y; ab[k].z += d.z; ab[k].w += d.w;
    }
    s1 = wave_sum(s1) * invw;
    s2 = wave_sum(s2) * invw;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = 4 * lane + 256 * k;
      const float4 v = make_float4(r * (g[k].x - s1 - xh[k].x * s2), r * (g[k].y - s1 - xh[k].y * s2),
                                   r * (g[k].z - s1 - xh[k].z * s2), r * (g[k].w - s1 - xh[k].w * s2));
      st4(ds_out + n * W + c, v);
      ad[k].x += v.x; ad[k].y += v.y; ad[k].z += v.z; ad[k].w += v.w;
    }
  }
  float* mine = smem + (size_t)wave * 3 * W;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    st4(mine + c, ag[k]);
    st4(mine + W + c, ab[k]);
    st4(mine + 2 * W + c, ad[k]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 3 * W; e += 256)
    part[(int64_t)blockIdx.x * 3 * W + e] = ((smem[e] + smem[3 * W + e]) + smem[6 * W + e]) + smem[9 * W + e];
}

// ---------------------------------------------------------------------------------------------------------
// element-wise epilogues
// ---------------------------------------------------------------------------------------------------------
// column sums (bias gradients, LayerNorm gamma/beta gradients): partials per SR_CS_ROWS rows, then a fixed-order fold
// ---------------------------------------------------------------------------------------------------------
// part[blk][c]      = sum_r a[r][c]                       (mode 0)
// part[blk][c]      = sum_r dy[r][c] * xh[r][c]           (mode 1: gamma gradient; xh from s, mean, rstd)
__global__ __launch_bounds__(256) void sr_colsum_kernel(const float* __restrict__ a, const float* __restrict__ s,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        int64_t T, int W, int mode, float* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * SR_CS_ROWS;
  const int64_t r1 = (r0 + SR_CS_ROWS < T) ? r0 + SR_CS_ROWS : T;
  for (int c = threadIdx.x; c < W; c += 256) {
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      float v = a[r * W + c];
      if (mode == 1) v *= (s[r * W + c] - mean[r]) * rstd[r];
      acc += v;
    }
    part[(int64_t)blockIdx.x * W + c] = acc;
  }
}
// LayerNorm parameter gradients in ONE pass over dy: part[blk][c] = sum_r dy xhat, part[blk][W + c] = sum_r dy
__global__ __launch_bounds__(256) void sr_colsum_ln_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           int64_t T, int W, float* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * SR_CS_ROWS;
  const int64_t r1 = (r0 + SR_CS_ROWS < T) ? r0 + SR_CS_ROWS : T;
  for (int c = threadIdx.x; c < W; c += 256) {
    float ag = 0.f, ab = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      const float g = dy[r * W + c];
      ag += g * ((s[r * W + c] - mean[r]) * rstd[r]);
      ab += g;
    }
    part[(int64_t)blockIdx.x * 2 * W + c] = ag;
    part[(int64_t)blockIdx.x * 2 * W + W + c] = ab;
  }
}
// the same with 16-byte accesses (W % 4 == 0, W <= 1024): SR_LB_ROWS rows per workgroup, a wave every 4th row, a lane the
// float4 chunks lane, lane + 64, ...; the four waves' partials are folded in fixed order through LDS
__global__ __launch_bounds__(256) void sr_colsum_ln_v4_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              int64_t T, int W, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4 waves][2][W]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SR_LB_ROWS;
  const int64_t r1 = (r0 + SR_LB_ROWS < T) ? r0 + SR_LB_ROWS : T;
  const int nq = W / 4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ag[4] = {z4, z4, z4, z4}, ab[4] = {z4, z4, z4, z4};
  for (int64_t n = r0 + wave; n < r1; n += 4) {
    const float m = mean[n], r = rstd[n];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qd = lane + 64 * k;
      if (qd < nq) {
        const float4 g = ld4(dy + n * W + 4 * qd), sv = ld4(s + n * W + 4 * qd);
        ag[k].x += g.x * ((sv.x - m) * r); ag[k].y += g.y * ((sv.y - m) * r);
        ag[k].z += g.z * ((sv.z - m) * r); ag[k].w += g.w * ((sv.w - m) * r);
        ab[k].x += g.x; ab[k].y += g.y; ab[k].z += g.z; ab[k].w += g.w;
      }
    }
  }
  float* mine = smem + (size_t)wave * 2 * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qd = lane + 64 * k;
    if (qd < nq) {
      st4(mine + 4 * qd, ag[k]);
      st4(mine + W + 4 * qd, ab[k]);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * W; e += 256)
    part[(int64_t)blockIdx.x * 2 * W + e] = ((smem[e] + smem[2 * W + e]) + smem[4 * W + e]) + smem[6 * W + e];
}
// dst[c] = sum over nparts partials (canonical order)
__global__ __launch_bounds__(256) void sr_fold_kernel(const float* __restrict__ part, int64_t stride, int nparts, int len,
                                                      float* __restrict__ dst) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  sm[grp][lane] = (c < len) ? strided_sum(part + c, stride, nparts, grp) : 0.f;
  __syncthreads();
  if (grp == 0 && c < len) dst[c] = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

// the same for MANY partials (row-block partials of the LayerNorm / column-sum kernels: hundreds to thousands): 16 columns
// per workgroup, 16 groups of threads each summing every 16th partial in order, fixed-order combine - 4x the workgroups
// and 4x shorter serial chains than sr_fold_kernel
__global__ __launch_bounds__(256) void sr_fold16_kernel(const float* __restrict__ part, int64_t stride, int nparts, int len,
                                                        float* __restrict__ dst) {
  __shared__ float sm[16][16];
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float a = 0.f;
  if (c < len) {
#pragma unroll 8
    for (int k = grp; k < nparts; k += 16) a += part[(int64_t)k * stride + c];
  }
  sm[grp][cl] = a;
  __syncthreads();
  if (grp == 0 && c < len) {
    float t = sm[0][cl];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += sm[g][cl];
    dst[c] = t;
  }
}
// every queued fold of a backward in one launch (SrFoldQueue, ultr_sr_rows.h): workgroup -> job by blk_begin, then the job's own order
__global__ __launch_bounds__(256) void sr_fold_all_kernel(SrFoldTable t) {
  __shared__ float sm[256];
  int j = 0;
  while (j + 1 < t.n && (int)blockIdx.x >= t.job[j + 1].blk_begin) ++j;
  const SrFoldJob jb = t.job[j];
  const int b = (int)blockIdx.x - jb.blk_begin;
  if (jb.wide == 2) {
    // many partials of a long vector (the per-workgroup partials of ultr_sr_bwd.hip: 256 x 66 - 125 KB): the 16-group order of the
    // `wide` form with FOUR columns per thread - a workgroup reads whole 256-byte runs of a partial instead of 64-byte pieces whose
    // other halves a workgroup on another XCD fetched again (45 -> 2x fewer bytes from HBM); same sums, same order per column
    const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int c = b * 64 + 4 * cl;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < jb.len) {
#pragma unroll 8
      for (int k = grp; k < jb.nparts; k += 16) {
        const float4 v = ld4(jb.part + (int64_t)k * jb.stride + c);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
    }
    __shared__ float4 sm4[256];
    sm4[grp * 16 + cl] = a;
    __syncthreads();
    if (grp == 0 && c < jb.len) {
      float4 v = sm4[cl];
#pragma unroll
      for (int g = 1; g < 16; ++g) {
        const float4 w = sm4[g * 16 + cl];
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
      const float o[4] = {v.x, v.y, v.z, v.w};  // (the destination sits at any float offset of the gradient vector)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < jb.len) jb.dst[c + i] = o[i];
    }
  } else if (jb.wide) {
    const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int c = b * 16 + cl;
    float a = 0.f;
    if (c < jb.len) {
#pragma unroll 8
      for (int k = grp; k < jb.nparts; k += 16) a += jb.part[(int64_t)k * jb.stride + c];
    }
    sm[grp * 16 + cl] = a;
    __syncthreads();
    if (grp == 0 && c < jb.len) {
      float v = sm[cl];
#pragma unroll
      for (int g = 1; g < 16; ++g) v += sm[g * 16 + cl];
      jb.dst[c] = v;
    }
  } else {
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = b * 64 + lane;
    sm[grp * 64 + lane] = (c < jb.len) ? strided_sum(jb.part + c, jb.stride, jb.nparts, grp) : 0.f;
    __syncthreads();
    if (grp == 0 && c < jb.len) jb.dst[c] = ((sm[lane] + sm[64 + lane]) + sm[128 + lane]) + sm[192 + lane];
  }
}
// width-1 output (the scorer, SetRank.py:136): y[t] = x[t] . w + b, one wavefront per row, 4 rows per workgroup
__global__ __launch_bounds__(256) void sr_rowdot_kernel(const float* __restrict__ X, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int64_t T, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(X[t * K + k], w[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[t] = acc + (bias != nullptr ? bias[0] : 0.f);
}
// its weight gradient: part[blk][k] = sum over SR_CS_ROWS rows of dy[t] X[t][k]
__global__ __launch_bounds__(256) void sr_colsum_w_kernel(const float* __restrict__ dy, const float* __restrict__ X, int64_t T,
                                                          int K, float* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * SR_CS_ROWS;
  const int64_t r1 = (r0 + SR_CS_ROWS < T) ? r0 + SR_CS_ROWS : T;
  for (int c = threadIdx.x; c < K; c += 256) {
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) acc = fmaf(dy[r], X[r * K + c], acc);
    part[(int64_t)blockIdx.x * K + c] = acc;
  }
}

// The scorer's backward in ONE pass over oh [T, K] (K = dff <= 256): G[t][k] = oh[t][k] > 0 ? dy[t] * w[k] : 0 (the dgrad
// through the width-1 Linear and the ReLU in front of it), part[blk] = { sum_t dy[t] oh[t][k] (d w) | sum_t dy[t] (d b) } per
// SR_CS_ROWS rows.  Replaces three launches (weighted column sums with a quarter of the lanes busy, a column sum of one
// column, a generic [T, 1] x [1, K] product): 64 -> ~15 us at config 5.  A wave takes every fourth row, a lane every 64th
// column; the four waves' partials are combined in fixed order.
__global__ __launch_bounds__(256) void sr_head_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ oh,
                                                          const float* __restrict__ w, int64_t T, int K, float* __restrict__ G,
                                                          float* __restrict__ part) {
  __shared__ float sm[4][260];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SR_CS_ROWS;
  const int64_t r1 = (r0 + SR_CS_ROWS < T) ? r0 + SR_CS_ROWS : T;
  float wv[4], aw[4] = {0.f, 0.f, 0.f, 0.f}, ab = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) wv[k] = (lane + 64 * k < K) ? w[lane + 64 * k] : 0.f;
  for (int64_t r = r0 + wave; r < r1; r += 4) {
    const float d = dy[r];
    ab += d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = lane + 64 * k;
      if (c < K) {
        const float x = oh[r * K + c];
        aw[k] = fmaf(d, x, aw[k]);
        G[r * K + c] = (x > 0.f) ? d * wv[k] : 0.f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < K) sm[wave][lane + 64 * k] = aw[k];
  if (lane == 0) sm[wave][256] = ab;
  __syncthreads();
  float* dst = part + (int64_t)blockIdx.x * (K + 1);
  for (int c = threadIdx.x; c < K; c += 256) dst[c] = ((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c];
  if (threadIdx.x == 0) dst[K] = ((sm[0][256] + sm[1][256]) + sm[2][256]) + sm[3][256];
}

}  // namespace

void SrFoldQueue::add(const float* part, int64_t stride, int nparts, int len, float* dst, hipStream_t st, bool own_buffer) {
  const bool wide = nparts >= 256;
  const bool in_arena = part >= arena && part < arena + cap;
  if ((in_arena || own_buffer) && tab.n < SR_MAX_FOLDS) {
    SrFoldJob& j = tab.job[tab.n++];
    // (a partial is a 16-byte-aligned run of `stride` = 4 k floats and `part` starts 4 m floats into it: the last float4 of a row stays inside)
    const bool vec4 = wide && len >= 1024 && (stride & 3) == 0 && ((uintptr_t)part & 15) == 0;
    j.part = part; j.dst = dst; j.stride = stride; j.nparts = nparts; j.len = len; j.wide = vec4 ? 2 : (wide ? 1 : 0);
    j.blk_begin = tab.nblocks;
    tab.nblocks += (wide && !vec4) ? (len + 15) / 16 : (len + 63) / 64;
    return;
  }
  if (wide) hipLaunchKernelGGL(sr_fold16_kernel, dim3((len + 15) / 16), dim3(256), 0, st, part, stride, nparts, len, dst);
  else hipLaunchKernelGGL(sr_fold_kernel, dim3((len + 63) / 64), dim3(256), 0, st, part, stride, nparts, len, dst);
}
void SrFoldQueue::flush(hipStream_t st) {
  if (tab.n > 0) hipLaunchKernelGGL(sr_fold_all_kernel, dim3(tab.nblocks), dim3(256), 0, st, tab);
  tab.n = 0; tab.nblocks = 0; used = 0;
}

void sr_rowdot(const float* X, const float* w, const float* bias, float* y, int64_t T, int K, hipStream_t st) {
  hipLaunchKernelGGL(sr_rowdot_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, X, w, bias, y, T, K);
}
void sr_colsum_w(const SrCall& c, const float* dy, const float* X, int K, float* dst) {  // partials per SR_CS_ROWS rows
                 float* cpart = c.folds->scratch(c.ws + c.p.ws_part, (int64_t)c.p.n_cs * K);
  hipLaunchKernelGGL(sr_colsum_w_kernel, dim3(c.p.n_cs), dim3(256), 0, c.st, dy, X, c.p.T, K, cpart);
  c.folds->add(cpart, (int64_t)K, c.p.n_cs, K, dst, c.st);
}
void sr_head_bwd(const SrCall& c, const float* dy, const float* oh, const float* w, int K, float* G, float* dst) {
  float* hpart = c.folds->scratch(c.ws + c.p.ws_part, (int64_t)c.p.n_cs * (K + 1));
  hipLaunchKernelGGL(sr_head_bwd_kernel, dim3(c.p.n_cs), dim3(256), 0, c.st, dy, oh, w, c.p.T, K, G, hpart);
  c.folds->add(hpart, (int64_t)K + 1, c.p.n_cs, K + 1, dst, c.st);
}
void sr_colsum(const SrCall& c, const float* a, const float* s, const float* mean, const float* rstd, int W, int mode, float* dst) {
  float* part = c.folds->scratch(c.ws + c.p.ws_part, (int64_t)c.p.n_cs * W);
  hipLaunchKernelGGL(sr_colsum_kernel, dim3(c.p.n_cs), dim3(256), 0, c.st, a, s, mean, rstd, c.p.T, W, mode, part);
  c.folds->add(part, (int64_t)W, c.p.n_cs, W, dst, c.st);
}

void sr_ln_gather_fwd(const float* feats, const int32_t* docids, int64_t n_docs, int batch, int L, int64_t T, int W, const float* gamma,
                      const float* beta, float* xg, float* y, float* mean_out, float* rstd_out, hipStream_t st) {
  const unsigned rblk = (unsigned)((T + SR_ROWS - 1) / SR_ROWS);
  if (W % 4 == 0 && W <= 1024 && ((uintptr_t)feats & 15) == 0)
    hipLaunchKernelGGL(sr_ln_gather_v4_kernel, dim3(rblk), dim3(SR_ROWS * 64), 0, st, feats, docids, n_docs, batch, L, T, W, gamma, beta, xg, y,
                       mean_out, rstd_out);
  else
    hipLaunchKernelGGL(sr_ln_fwd_kernel, dim3(rblk), dim3(SR_ROWS * 64), 0, st, feats, (const float*)nullptr, (const float*)nullptr, docids, n_docs,
                       batch, L, T, W, gamma, beta, xg, y, mean_out, rstd_out);
}
void sr_ln_bwd_rows(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma, int W, float* dx) {
  hipLaunchKernelGGL(sr_ln_bwd_kernel, dim3((unsigned)((c.p.T + SR_ROWS - 1) / SR_ROWS)), dim3(SR_ROWS * 64), 0, c.st, dy, s, mean, rstd, gamma,
                     c.p.T, W, dx);
}
// residual LayerNorm forward: y = LN(a + (b + bias)); float4 kernel when the rows allow it
void sr_ln_residual_fwd(const float* a, const float* b, const float* bias, int64_t T, int W, const float* gamma, const float* beta,
                        float* sum_out, float* y, float* mean_out, float* rstd_out, int batch, int L, hipStream_t st) {
  const unsigned rblk = (unsigned)((T + SR_ROWS - 1) / SR_ROWS);
  const bool v4 = (W == 256 || W == 512 || W == 768 || W == 1024) &&
                  ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)sum_out | (uintptr_t)y) & 15) == 0);  // b / sum_out may be NULL
  if (v4 && W == 256) hipLaunchKernelGGL(sr_ln_fwd_v4_kernel<1>, dim3(rblk), dim3(SR_ROWS * 64), 0, st, a, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4 && W == 512) hipLaunchKernelGGL(sr_ln_fwd_v4_kernel<2>, dim3(rblk), dim3(SR_ROWS * 64), 0, st, a, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4 && W == 768) hipLaunchKernelGGL(sr_ln_fwd_v4_kernel<3>, dim3(rblk), dim3(SR_ROWS * 64), 0, st, a, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4) hipLaunchKernelGGL(sr_ln_fwd_v4_kernel<4>, dim3(rblk), dim3(SR_ROWS * 64), 0, st, a, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else
    hipLaunchKernelGGL(sr_ln_fwd_kernel, dim3(rblk), dim3(SR_ROWS * 64), 0, st, a, b, bias, (const int32_t*)nullptr, (int64_t)0, batch, L, T, W,
                       gamma, beta, sum_out, y, mean_out, rstd_out);
}

// dst[0..W) = d gamma, dst[W..2W) = d beta (adjacent in the flat layout: <ln>.weight then <ln>.bias)
// dx = LayerNorm backward of dy; dst_gb = dgamma | dbeta; dst_bias = column sums of dx (may be NULL).  W <= 1024.
int sr_ln_bwd_cs(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma, int W,
                 float* dx, float* dst_gb, float* dst_bias) {
  const SrPlan& p = c.p;
  hipStream_t st = c.st;
  float* part = c.folds->scratch(c.ws + p.ws_part, (int64_t)p.n_lb * 3 * W);
  const size_t lds = (size_t)4 * 3 * W * sizeof(float);
  const bool v4 = (W == 256 || W == 512) && ((((uintptr_t)dy | (uintptr_t)s | (uintptr_t)dx) & 15) == 0);
  if (v4 && W == 256) hipLaunchKernelGGL(sr_ln_bwd_cs_v4_kernel<1>, dim3(p.n_lb), dim3(256), lds, st, dy, s, mean, rstd, gamma, p.T, dx, part);
  else if (v4) hipLaunchKernelGGL(sr_ln_bwd_cs_v4_kernel<2>, dim3(p.n_lb), dim3(256), lds, st, dy, s, mean, rstd, gamma, p.T, dx, part);
  else if (W <= 256) hipLaunchKernelGGL(sr_ln_bwd_cs_kernel<4>, dim3(p.n_lb), dim3(256), lds, st, dy, s, mean, rstd, gamma, p.T, W, dx, part);
  else hipLaunchKernelGGL(sr_ln_bwd_cs_kernel<16>, dim3(p.n_lb), dim3(256), lds, st, dy, s, mean, rstd, gamma, p.T, W, dx, part);
  c.folds->add(part, (int64_t)3 * W, p.n_lb, 2 * W, dst_gb, st);
  if (dst_bias != nullptr) c.folds->add(part + 2 * W, (int64_t)3 * W, p.n_lb, W, dst_bias, st);  // (NULL: a dropout site sits between ds and the bias)
  return 0;
}
void sr_colsum_ln(const SrCall& c, const float* dy, const float* s, const float* mean, const float* rstd, int W, float* dst) {
  const SrPlan& p = c.p;
  hipStream_t st = c.st;
  float* part = c.folds->scratch(c.ws + p.ws_part, (int64_t)p.n_lb * 2 * W);  // n_lb >= n_cs
  if (W % 4 == 0 && W <= 1024 && ((((uintptr_t)dy | (uintptr_t)s) & 15) == 0)) {
    hipLaunchKernelGGL(sr_colsum_ln_v4_kernel, dim3(p.n_lb), dim3(256), (size_t)8 * W * sizeof(float), st, dy, s, mean, rstd, p.T, W, part);
    c.folds->add(part, (int64_t)2 * W, p.n_lb, 2 * W, dst, st);
    return;
  }
  hipLaunchKernelGGL(sr_colsum_ln_kernel, dim3(p.n_cs), dim3(256), 0, st, dy, s, mean, rstd, p.T, W, part);
  c.folds->add(part, (int64_t)2 * W, p.n_cs, 2 * W, dst, st);
}

