// ultr_sr_dropout.hip - the row kernels of SetRank's dropout steps (ultr_sr_dropout.h has the mask law).  A dropout step runs the
// separate-launch paths of ultr_setrank.hip in both directions; these kernels stand where sr_ln_residual_fwd / the bias column sums of
// sr_ln_bwd_cs (ultr_sr_rows.hip) stand at rate 0.  One Philox call covers four neighbouring columns of one token, so every kernel walks rows in quads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_sr_dropout.h"

#define SR_DROP_EPS 1e-6f  // nn.LayerNorm(eps=1e-6), as ultr_sr_plan.h's SR_EPS
#define SR_DROP_WAVES 4    // rows per workgroup of the LayerNorm kernels (one wavefront per row)

namespace {

// the law's token of kernel row n = b L + l
__device__ __forceinline__ uint32_t drop_token(int64_t n, int B, int L) {
  const int b = (int)(n / L), l = (int)(n - (int64_t)b * L);
  return (uint32_t)l * (uint32_t)B + (uint32_t)b;
}
// the multipliers (scale or 0) of columns 4 q .. 4 q + 3 of token t
__device__ __forceinline__ float4 drop_quad(const SrDropArgs& a, uint32_t c1, uint32_t t, uint32_t q) {
  const Philox rng{a.k0, a.k1};
  uint32_t c[4] = {t, c1, q, SR_DROPOUT_TAG};
  rng(c);
  return make_float4(u01(c[0]) >= a.rate ? a.scale : 0.f, u01(c[1]) >= a.rate ? a.scale : 0.f, u01(c[2]) >= a.rate ? a.scale : 0.f,
                     u01(c[3]) >= a.rate ? a.scale : 0.f);
}
__device__ __forceinline__ float pick(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// the general form (any W): lane owns the quads lane, lane + 64, ...; up to 1024 columns the row stays in registers between the
// passes, beyond that the later passes read the pre-norm sum back from sum_out (written by the same thread)
__global__ __launch_bounds__(SR_DROP_WAVES * 64) void sr_drop_ln_fwd_kernel(SrDropArgs a, uint32_t c1, const float* x, const float* b /* may alias y */,
                                                                           const float* __restrict__ bias, int64_t T, int W,
                                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                           float* __restrict__ sum_out, float* y, float* __restrict__ mean_out,
                                                                           float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_DROP_WAVES + wave;
  if (n >= T) return;
  const uint32_t t = drop_token(n, a.B, a.L);
  const int nq = (W + 3) >> 2;
  if (W <= 1024) {
    float v[4][4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = lane + 64 * k;
      float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < nq) m = drop_quad(a, c1, t, (uint32_t)q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        v[k][j] = 0.f;
        if (c < W) {
          v[k][j] = x[n * W + c] + (b[n * W + c] + bias[c]) * pick(m, j);
          sum_out[n * W + c] = v[k][j];
        }
        s += v[k][j];
      }
    }
    const float mean = wave_sum(s) / (float)W;
    float qq = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dlt = (4 * (lane + 64 * k) + j < W) ? v[k][j] - mean : 0.f;
        qq += dlt * dlt;
      }
    const float rstd = 1.0f / sqrtf(wave_sum(qq) / (float)W + SR_DROP_EPS);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * (lane + 64 * k) + j;
        if (c < W) y[n * W + c] = (v[k][j] - mean) * rstd * gamma[c] + beta[c];
      }
    if (lane == 0) {
      mean_out[n] = mean;
      rstd_out[n] = rstd;
    }
    return;
  }
  float s = 0.f;
  for (int q = lane; q < nq; q += 64) {
    const float4 m = drop_quad(a, c1, t, (uint32_t)q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      if (c < W) {
        const float v = x[n * W + c] + (b[n * W + c] + bias[c]) * pick(m, j);
        sum_out[n * W + c] = v;
        s += v;
      }
    }
  }
  const float mean = wave_sum(s) / (float)W;
  float qq = 0.f;
  for (int q = lane; q < nq; q += 64)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      if (c < W) {
        const float dlt = sum_out[n * W + c] - mean;
        qq += dlt * dlt;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(qq) / (float)W + SR_DROP_EPS);
  for (int q = lane; q < nq; q += 64)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      if (c < W) y[n * W + c] = (sum_out[n * W + c] - mean) * rstd * gamma[c] + beta[c];
    }
  if (lane == 0) {
    mean_out[n] = mean;
    rstd_out[n] = rstd;
  }
}

// W = NV * 256 with 16-byte accesses, as sr_ln_fwd_v4_kernel (ultr_sr_rows.hip): lane owns columns 4 lane .. 4 lane + 3 (+ 256 k) = quad lane + 64 k
template <int NV>
__global__ __launch_bounds__(SR_DROP_WAVES * 64) void sr_drop_ln_fwd_v4_kernel(SrDropArgs a, uint32_t c1, const float* x, const float* b /* may alias y */,
                                                                              const float* __restrict__ bias, int64_t T,
                                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                              float* __restrict__ sum_out, float* y, float* __restrict__ mean_out,
                                                                              float* __restrict__ rstd_out) {
  constexpr int W = NV * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * SR_DROP_WAVES + wave;
  if (n >= T) return;
  const uint32_t t = drop_token(n, a.B, a.L);
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    const float4 xv = ld4(x + n * W + c), bv = ld4(b + n * W + c);
    const float4 m = drop_quad(a, c1, t, (uint32_t)(lane + 64 * k));
    v[k] = make_float4(xv.x + (bv.x + bias[c]) * m.x, xv.y + (bv.y + bias[c + 1]) * m.y, xv.z + (bv.z + bias[c + 2]) * m.z,
                       xv.w + (bv.w + bias[c + 3]) * m.w);  // parameters: any float offset
    st4(sum_out + n * W + c, v[k]);
    s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + SR_DROP_EPS);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    st4(y + n * W + c, make_float4((v[k].x - mean) * rstd * gamma[c] + beta[c], (v[k].y - mean) * rstd * gamma[c + 1] + beta[c + 1],
                                   (v[k].z - mean) * rstd * gamma[c + 2] + beta[c + 2], (v[k].w - mean) * rstd * gamma[c + 3] + beta[c + 3]));
  }
  if (lane == 0) {
    mean_out[n] = mean;
    rstd_out[n] = rstd;
  }
}

// dst = D(src), and the column sums of dst per SR_DROP_ROWS rows (the bias gradient of the Linear in front of the site).  A wave
// takes every fourth row of the workgroup's rows, a lane the quads lane, lane + 64, ... of a 1024-column chunk; the four waves'
// column partials are folded in fixed order through LDS, chunk by chunk.  VEC: W % 4 == 0 and 16-byte aligned buffers.
template <bool VEC>
__global__ __launch_bounds__(256) void sr_drop_mask_kernel(SrDropArgs a, uint32_t c1, const float* src, float* dst, float* __restrict__ part,
                                                           int64_t T, int W) {
  __shared__ __attribute__((aligned(16))) float sm[4][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SR_DROP_ROWS;
  const int64_t r1 = (r0 + SR_DROP_ROWS < T) ? r0 + SR_DROP_ROWS : T;
  const int nq = (W + 3) >> 2;
  for (int qb = 0; qb < nq; qb += 256) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[4] = {z4, z4, z4, z4};
    for (int64_t n = r0 + wave; n < r1; n += 4) {
      const uint32_t t = drop_token(n, a.B, a.L);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = qb + lane + 64 * k;
        if (q < nq) {
          const float4 m = drop_quad(a, c1, t, (uint32_t)q);
          const int c = 4 * q;
          float4 o;
          if constexpr (VEC) {
            const float4 v = ld4(src + n * W + c);
            o = make_float4(v.x * m.x, v.y * m.y, v.z * m.z, v.w * m.w);
            st4(dst + n * W + c, o);
          } else {
            o = z4;
            o.x = src[n * W + c] * m.x;
            dst[n * W + c] = o.x;
            if (c + 1 < W) { o.y = src[n * W + c + 1] * m.y; dst[n * W + c + 1] = o.y; }
            if (c + 2 < W) { o.z = src[n * W + c + 2] * m.z; dst[n * W + c + 2] = o.z; }
            if (c + 3 < W) { o.w = src[n * W + c + 3] * m.w; dst[n * W + c + 3] = o.w; }
          }
          acc[k].x += o.x; acc[k].y += o.y; acc[k].z += o.z; acc[k].w += o.w;
        }
      }
    }
    if (part == nullptr) continue;  // (kernel argument: the whole workgroup takes the same way)
#pragma unroll
    for (int k = 0; k < 4; ++k) st4(&sm[wave][4 * (lane + 64 * k)], acc[k]);
    __syncthreads();
    const int c0 = 4 * qb;
    const int len = (W - c0 < 1024) ? W - c0 : 1024;
    for (int e = threadIdx.x; e < len; e += 256) part[(int64_t)blockIdx.x * W + c0 + e] = ((sm[0][e] + sm[1][e]) + sm[2][e]) + sm[3][e];
    __syncthreads();
  }
}

}  // namespace

int sr_drop_args(float rate, uint64_t seed, uint64_t step, uint32_t stream, int B, int L, SrDropArgs* out) {
  if (!(rate >= 0.0f && rate < 1.0f) || B <= 0 || L <= 0 || stream >= (1u << 24) || out == nullptr) return ULTR_E_BADARG;
  const Philox key = philox_step_key(seed, step);
  out->k0 = key.k0;
  out->k1 = key.k1;
  out->stream = stream;
  out->rate = rate;
  out->scale = 1.0f / (1.0f - rate);
  out->B = B;
  out->L = L;
  return 0;
}

void sr_drop_ln_fwd_launch(const SrDropArgs& a, int site, const float* x, const float* b, const float* bias, int64_t T, int W,
                           const float* gamma, const float* beta, float* sum_out, float* y, float* mean_out, float* rstd_out,
                           hipStream_t st) {
  const unsigned rblk = (unsigned)((T + SR_DROP_WAVES - 1) / SR_DROP_WAVES);
  const dim3 blk(SR_DROP_WAVES * 64);
  const uint32_t c1 = (a.stream << 8) | (uint32_t)site;
  const bool v4 = (W == 256 || W == 512 || W == 768 || W == 1024) && ((((uintptr_t)x | (uintptr_t)b | (uintptr_t)sum_out | (uintptr_t)y) & 15) == 0);
  if (v4 && W == 256) hipLaunchKernelGGL(sr_drop_ln_fwd_v4_kernel<1>, dim3(rblk), blk, 0, st, a, c1, x, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4 && W == 512) hipLaunchKernelGGL(sr_drop_ln_fwd_v4_kernel<2>, dim3(rblk), blk, 0, st, a, c1, x, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4 && W == 768) hipLaunchKernelGGL(sr_drop_ln_fwd_v4_kernel<3>, dim3(rblk), blk, 0, st, a, c1, x, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else if (v4) hipLaunchKernelGGL(sr_drop_ln_fwd_v4_kernel<4>, dim3(rblk), blk, 0, st, a, c1, x, b, bias, T, gamma, beta, sum_out, y, mean_out, rstd_out);
  else hipLaunchKernelGGL(sr_drop_ln_fwd_kernel, dim3(rblk), blk, 0, st, a, c1, x, b, bias, T, W, gamma, beta, sum_out, y, mean_out, rstd_out);
}

void sr_drop_mask_launch(const SrDropArgs& a, int site, const float* src, float* dst, float* part, int64_t T, int W, hipStream_t st) {
  const uint32_t c1 = (a.stream << 8) | (uint32_t)site;
  const unsigned nblk = (unsigned)sr_drop_parts(T);
  const bool vec = W % 4 == 0 && ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
  if (vec) hipLaunchKernelGGL(sr_drop_mask_kernel<true>, dim3(nblk), dim3(256), 0, st, a, c1, src, dst, part, T, W);
  else hipLaunchKernelGGL(sr_drop_mask_kernel<false>, dim3(nblk), dim3(256), 0, st, a, c1, src, dst, part, T, W);
}
