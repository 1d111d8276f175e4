// ultr_setrank.hip — the SetRank ranking model (reference ultra/ranking_model/SetRank.py:23-255),
// forward and backward.  Everything is a kernel of this library (no vendor BLAS):
//   * the token-local Linear layers run on the LDS-tiled fp32 matrix-core GEMM of ultr_gemm.h: forward Y = X.W^T + b
//     (+ReLU) with the reference's [out, in] weights as the n-major operand and the bias / activation in the epilogue,
//     dgrad dX (+)= dY.W with the accumulate / ReLU-mask epilogue; the two M = 1 products of the scorer have row kernels;
//   * weight gradients here (sr_wgrad_kernel: 64 x 64 blocks x row chunks -> slabs) and the split-half planes of the weights;
//     feature gather + LayerNorm, residual + LayerNorm (forward, and backward fused with the gamma / beta / bias column sums),
//     column sums and folds in ultr_sr_rows.hip; the per-(list, head) self-attention WITHOUT Q/K/V projections (the heads are
//     slices of x itself, SetRank.py:57-66) in ultr_sr_attn.hip; the fused forward kernels of round 5 in ultr_sr_block.hip, the
//     persistent launches of the encoder blocks in ultr_sr_fwd.hip / ultr_sr_bwd.hip (round 6);
//   * deterministic: no atomics; every partial sum (slabs, row-block partials) is folded in a fixed order, all folds of a
//     backward in ONE launch at its end (sr_fold_all_kernel);
//   * no state between or beside calls: ultr_setrank_forward / _backward build ONE SrCall on their stack (plan, parameters, split-half
//     planes, a copy of the knobs, CU count, buffers, stream, the backward's SrFoldQueue) and every host helper takes it;
//   * which launches a step takes is decided ONCE per call, before its first launch: the route (SrRoute, ultr_sr_plan.h, next to the
//     plan and the knobs) - the two functions at the end of this file only read it.
// Token n = b*L + l (list-major), all activations row-major [T, width].  Parameters: ONE flat vector in the
// reference's state_dict order (ultr_setrank_param_offsets).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#ifdef ULTR_TRACE
__device__ unsigned long long g_ugemm_trace[64 * 32];
#define UGEMM_TRACE_STAMP(slot)                                                                    \
  do {                                                                                             \
    if (threadIdx.x == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64 && g_ugemm_trace[(blockIdx.x >> 3) * 32 + 31] == 0ull) \
      g_ugemm_trace[(blockIdx.x >> 3) * 32 + (slot)] = __builtin_amdgcn_s_memtime();              \
  } while (0)
extern "C" int ultr_gemm_trace_read(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_ugemm_trace), sizeof(unsigned long long) * 64 * 32);
}
unsigned long long* sr_gemm_trace_slots() {  // for sr_block_fwd_kernel (ultr_sr_block.hip: another code object), which stamps slots 20 .. 30
  void* p = nullptr;
  return hipGetSymbolAddress(&p, HIP_SYMBOL(g_ugemm_trace)) == hipSuccess ? (unsigned long long*)p : nullptr;
}
extern "C" int ultr_gemm_trace_arm(int on) {  // slot 31 != 0: frozen
  unsigned long long z[64 * 32];
  for (int k = 0; k < 64 * 32; ++k) z[k] = (on || (k & 31) != 31) ? 0ull : 1ull;
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ugemm_trace), z, sizeof(z));
}
#endif
#ifndef UGEMM_TRACE_STAMP
#define UGEMM_TRACE_STAMP(slot) \
  do {                          \
  } while (0)
#endif
#include "ultr_gemm.h"
#include "ultr_h3.h"
#include "ultr_plan.h"
#include "ultr_sr_attn.h"
#include "ultr_sr_bwd.h"
#include "ultr_sr_dropout.h"
#include "ultr_sr_plan.h"
#include "ultr_sr_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// weight gradients of the plain Linears:  dW[M, K] = dY[T, M]^T X[T, K],  db[M] = column sums of dY
// ---------------------------------------------------------------------------------------------------------
// T is ~100k rows and the outputs are small (at most d x d), so the contraction is split over row chunks:
// workgroup = (64 x 64 output block, chunk); its four waves take a quarter of the chunk each, stream the two
// operand rows straight from global memory into MFMA fragments (lane (i, q): row 4 step + q, float4 at column 4 i -
// the four floats feed the four 16-wide sub-tiles, i.e. the block's columns are dealt round-robin to the
// sub-tiles, which the store undoes), 16 accumulator tiles per wave, a three-deep register ring of operands,
// then a fixed-order LDS reduction over the waves and one slab [M*K + M] per chunk; sr_fold_kernel sums the slabs.
// (rocBLAS ran these as strided-batched 32x32 macro-tiles at ~43 TFLOP/s; same design as dnn_wgrad_kernel.)
constexpr int SRW_SPT = 2;  // steps (of 4 rows) per trip
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void sr_wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ X, int64_t T, int M,
                                                       int K, int nkb, int nsplit, int rps, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float (*red)[64 * 64] = reinterpret_cast<float (*)[64 * 64]>(smem);
  float (*bred)[64] = reinterpret_cast<float (*)[64]>(smem + 4 * 64 * 64);
  const int split = blockIdx.x % nsplit, tile = blockIdx.x / nsplit;
  const int mb = tile / nkb, kb = tile - mb * nkb;
  const int m0 = mb * 64, k0 = kb * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int64_t n0 = (int64_t)split * rps;
  const int rows_here = (int)((n0 + rps < T) ? rps : T - n0);
  const int rpw = rps / 4;
  const int rbeg = wave * rpw;
  const int rend = (rbeg + rpw < rows_here) ? rbeg + rpw : rows_here;
  // descriptors cover exactly this chunk: a masked lane presents ULTR_OOB and reads 0
  const Src ys = make_src(dY + n0 * M, (int64_t)rows_here * M);
  const Src xs = make_src(X + n0 * K, (int64_t)rows_here * K);
  const unsigned mc = (unsigned)(m0 + 4 * i) * 4u, kc = (unsigned)(k0 + 4 * i) * 4u;
  const unsigned mstride = (unsigned)M * 4u, kstride = (unsigned)K * 4u;
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  struct StepRegs {
    float4 a, x;
  };
  // only dY must be exactly zero for rows outside the wave's slice; X rows there are other rows of the chunk (finite)
  auto load_step = [&](int r, StepRegs& sr) {
    sr.a = buf_ld4(ys, (r < rend) ? (unsigned)r * mstride + mc : ULTR_OOB);
    sr.x = buf_ld4(xs, (unsigned)r * kstride + kc);
  };
  int rr = rbeg;
  auto trip = [&](StepRegs(&cu)[SRW_SPT], StepRegs(&nx)[SRW_SPT]) {
#pragma unroll
    for (int u = 0; u < SRW_SPT; ++u) load_step(rr + 4 * SRW_SPT * 2 + 4 * u + q, nx[u]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < SRW_SPT; ++u) {
      const float4 a_c = cu[u].a, x_c = cu[u].x;
      bsum.x += a_c.x;
      bsum.y += a_c.y;
      bsum.z += a_c.z;
      bsum.w += a_c.w;
      const float av[4] = {a_c.x, a_c.y, a_c.z, a_c.w};
      const float bv[4] = {x_c.x, x_c.y, x_c.z, x_c.w};
#pragma unroll
      for (int ta = 0; ta < 4; ++ta)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = mfma16(av[ta], bv[tb], acc[ta][tb]);
    }
    rr += 4 * SRW_SPT;
  };
  const int ntrip = (rend - rbeg + 4 * SRW_SPT - 1) / (4 * SRW_SPT);
  StepRegs ra[SRW_SPT], rb[SRW_SPT], rc[SRW_SPT];
#pragma unroll
  for (int u = 0; u < SRW_SPT; ++u) {
    load_step(rbeg + 4 * u + q, ra[u]);
    load_step(rbeg + 4 * SRW_SPT + 4 * u + q, rb[u]);
  }
  int t = 0;
  for (; t + 2 < ntrip; t += 3) {
    trip(ra, rc);
    trip(rb, ra);
    trip(rc, rb);
  }
  if (t < ntrip) trip(ra, rc);
  if (t + 1 < ntrip) trip(rb, ra);
  // lane holds D_{ta,tb}[row = 4q + r][col = i]  ->  block-local (m = 4 (4q + r) + ta, k = 4 i + tb)
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ml = 4 * (4 * q + r) + ta;
      st4(&red[wave][ml * 64 + 4 * i], make_float4(acc[ta][0][r], acc[ta][1][r], acc[ta][2][r], acc[ta][3][r]));
    }
  {
    float4 sb = bsum;  // the 4 row groups q sit in lanes i, i+16, i+32, i+48
    sb.x = quad_sum(sb.x); sb.y = quad_sum(sb.y); sb.z = quad_sum(sb.z); sb.w = quad_sum(sb.w);
    if (q == 0) st4(&bred[wave][4 * i], sb);
  }
  __syncthreads();
  float* slab = part + (int64_t)split * ((int64_t)M * K + M);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = tid + 256 * it;  // float4 index inside the 64x64 block
    const int ml = e >> 4, k4 = (e & 15) * 4;
    const float4 v0 = ld4(&red[0][ml * 64 + k4]), v1 = ld4(&red[1][ml * 64 + k4]);
    const float4 v2 = ld4(&red[2][ml * 64 + k4]), v3 = ld4(&red[3][ml * 64 + k4]);
    float4 o;
    o.x = ((v0.x + v1.x) + v2.x) + v3.x;
    o.y = ((v0.y + v1.y) + v2.y) + v3.y;
    o.z = ((v0.z + v1.z) + v2.z) + v3.z;
    o.w = ((v0.w + v1.w) + v2.w) + v3.w;
    const int m = m0 + ml, k = k0 + k4;
    if (m < M && k < K) st4(slab + (int64_t)m * K + k, o);  // K % 4 == 0
  }
  if (kb == 0 && tid < 64 && m0 + tid < M)
    slab[(int64_t)M * K + m0 + tid] = ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// The token-local Linear layers (round 1: rocBLAS sgemm + separate bias / ReLU / mask passes) run on the library's own
// LDS-tiled matrix-core GEMM (ultr_gemm.h) with the bias, the ReLU, the ReLU mask of the backward and the accumulation
// into an existing gradient fused into the epilogue.  Shapes the vector path cannot take (contraction or row length not
// a multiple of 4, unaligned bases, single-column outputs) go through plain one-thread-per-output kernels: they only
// occur in toy configurations and for the width-1 scorer.
__global__ __launch_bounds__(256) void sr_gemm_xwT_ref_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ Y, int64_t T,
                                                              int K, int M, int relu) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= T * M) return;
  const int64_t t = e / M;
  const int m = (int)(e - t * M);
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(X[t * K + k], W[(int64_t)m * K + k], acc);
  if (bias != nullptr) acc += bias[m];
  Y[e] = relu ? fmaxf(acc, 0.f) : acc;
}
__global__ __launch_bounds__(256) void sr_gemm_dyw_ref_kernel(const float* __restrict__ dY, const float* __restrict__ W,
                                                              float* __restrict__ dX, const float* __restrict__ mask, int64_t T,
                                                              int K, int M, int accumulate) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= T * K) return;
  const int64_t t = e / K;
  const int k = (int)(e - t * K);
  float acc = accumulate ? dX[e] : 0.f;
  for (int m = 0; m < M; ++m) acc = fmaf(dY[t * M + m], W[(int64_t)m * K + k], acc);
  if (mask != nullptr && !(mask[e] > 0.f)) acc = 0.f;
  dX[e] = acc;
}
// part[chunk][m * K + k] = sum over the chunk's rows of dY[t][m] X[t][k]
__global__ __launch_bounds__(256) void sr_gemm_dyTx_ref_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                               float* __restrict__ part, int64_t rows, int K, int M) {
  const int64_t t0 = (int64_t)blockIdx.y * rows;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < M * K; e += gridDim.x * 256) {
    const int m = e / K, k = e - m * K;
    float acc = 0.f;
    for (int64_t t = t0; t < t0 + rows; ++t) acc = fmaf(dY[t * M + m], X[t * K + k], acc);
    part[(int64_t)blockIdx.y * M * K + e] = acc;
  }
}

// ---- split-half weight planes ------------------------------------------------------------------------------------------------
struct SrSplitTable {
  int n;
  SrPlan::SplitMat m[32];
};
// blockIdx.y = 4 * matrix + phase (0: the forward planes [M][ldK], 1: the transposed planes [K][ldM], 2: the fragment-major forward copy
// of the fused block kernel - ultr_h3_index - where the plan has one, 3: the fragment-major copy of the transpose for the fused backward
// launches); one element per thread
__global__ __launch_bounds__(256) void sr_split_planes_kernel(SrSplitTable tb, const float* __restrict__ params, _Float16* __restrict__ planes,
                                                              uint32_t* __restrict__ range_flag) {
  const SrPlan::SplitMat m = tb.m[blockIdx.y / 4];
  const int phase = blockIdx.y % 4;
  if (phase == 3) {  // fragment-major copy of W^T: output column k of W, contraction over m
    if (m.gt_off < 0) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m.K * m.ldM) return;
    const int k = (int)(e / m.ldM), mm = (int)(e - (int64_t)k * m.ldM);
    const float w = mm < m.M ? params[m.off + (int64_t)mm * m.K + k] * ULTR_H3_WSCALE : 0.f;
    const _Float16 hi = (_Float16)w, lo = (_Float16)(w - (float)hi);
    _Float16* dst = planes + m.gt_off;
    dst[ultr_h3_index(k, mm, m.ldM >> 5, 0)] = hi;
    dst[ultr_h3_index(k, mm, m.ldM >> 5, 1)] = lo;
    return;
  }
  if (phase == 2) {
    if (m.g_off < 0) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m.M * m.ldK) return;
    const int mm = (int)(e / m.ldK), k = (int)(e - (int64_t)mm * m.ldK);
    const float w = k < m.K ? params[m.off + (int64_t)mm * m.K + k] * ULTR_H3_WSCALE : 0.f;
    const _Float16 hi = (_Float16)w, lo = (_Float16)(w - (float)hi);
    _Float16* dst = planes + m.g_off;
    dst[ultr_h3_index(mm, k, m.ldK >> 5, 0)] = hi;
    dst[ultr_h3_index(mm, k, m.ldK >> 5, 1)] = lo;
    return;
  }
  const int rows = phase ? m.K : m.M, ld = phase ? m.ldM : m.ldK, cols = phase ? m.M : m.K;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)rows * ld) return;
  const int r = (int)(e / ld), c = (int)(e - (int64_t)r * ld);
  float w = 0.f;
  if (c < cols) w = params[m.off + (phase ? ((int64_t)c * m.K + r) : ((int64_t)r * m.K + c))] * UGEMM_H3_WSCALE;
  // |w| >= 64 raises ULTR_H3_FLAG_NEAR, >= 128 (or NaN: the planes overflow) ULTR_H3_FLAG_OVER - the step's update launch reports the word
  // (ultr_update_desc::range_flag) and the engine switches this model to the fp32 products
  if (!(fabsf(w) < 16384.0f)) flag_or(range_flag, !(fabsf(w) < 32768.0f) ? (ULTR_H3_FLAG_OVER | ULTR_H3_FLAG_NEAR) : ULTR_H3_FLAG_NEAR);
  const _Float16 hi = (_Float16)w, lo = (_Float16)(w - (float)hi);
  _Float16* dst = planes + (phase ? m.t_off : m.f_off);
  dst[e] = hi;
  dst[(int64_t)rows * ld + e] = lo;
}
// the knobs' storage (SrKnobs, ultr_sr_plan.h): read from the environment ONCE (first use), replaced whole by ultr_config_reload()
SrKnobs g_knobs = {};
void sr_knobs_load() {
  auto num = [](const char* s, int dflt) { return (s && *s) ? atoi(s) : dflt; };
  SrKnobs k;
  k.h3 = num(getenv("ULTR_SR_H3"), 1);
  k.attn_h3 = num(getenv("ULTR_SR_ATTN_H3"), 1);
  k.attn_mask = num(getenv("ULTR_SR_ATTN_H3_MASK"), -1);
  k.wg_h3 = num(getenv("ULTR_SR_WG_H3"), 1);
  k.bwd_fused = num(getenv("ULTR_SR_BWD_FUSED"), 7);
  k.attn_long_min = num(getenv("ULTR_SR_ATTN_LONG_MIN"), SR_ATTN_ONE_PASS_MAX + 1);
  k.block = num(getenv("ULTR_SR_BLOCK"), 3);
  if (k.block == 1) k.block = 2;  // (once the 16-wave form of sr_block_fwd_kernel)
  k.loaded = true;
  g_knobs = k;
}
const SrKnobs& sr_knobs() {
  if (!g_knobs.loaded) sr_knobs_load();
  return g_knobs;
}
// compute units of the current device (the row tiling of the persistent launches)
int sr_cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  return cus;
}

// activations (a, c) must be 16-byte aligned with rows a multiple of 4 floats (LDS staging and float4 stores); the weight
// matrix only needs its natural 4-byte alignment: in SetRank's flat parameter vector every encoder matrix sits at an odd
// float offset (the width-1 scorer bias precedes them), and buffer_load_dwordx4 takes dword-aligned addresses
bool vec_ok(const void* a, const void* c, int K, int ld_out) {
  return K % 4 == 0 && ld_out % 4 == 0 && ((((uintptr_t)a | (uintptr_t)c) & 15) == 0);
}
// the Linears below: X, Y, dY, dX are [T, .] with T = c.p.T, the weight W[M, K] sits at float offset `w` of the parameter vector
// row-major  Y[T, M] = act(X[T, K] . W[M, K]^T + bias)      (bias may be NULL; relu 0 / 1)
int gemm_xwT(const SrCall& c, const float* X, int64_t w, const float* bias, float* Y, int K, int M, int relu) {
  const int64_t T = c.p.T;
  const float* W = c.params + w;
  if (M >= 16 && vec_ok(X, Y, K, M) && T * (K > M ? K : M) * 4 < ((int64_t)1 << 31)) {
    const ugemm::APlain a{X, T, K, K};
    const ugemm::EBiasAct e{Y, bias, M, relu ? 1 : -1};
    if (const SrPlan::SplitMat* sm = c.split(w, M, K)) {  // split-half planes of W: the product on the fp16 matrix cores
      const ugemm::Dims dh{T, M, K, sm->ldK};
      const _Float16* hi = c.planes + sm->f_off;
      return ugemm::run_h3(dh, a, hi, hi + (int64_t)M * sm->ldK, e, c.st) == hipSuccess ? 0 : ULTR_E_UNSUPPORTED;
    }
    const ugemm::Dims d{T, M, K, K};
    return ugemm::run<true>(d, a, W, e, c.st) == hipSuccess ? 0 : ULTR_E_UNSUPPORTED;
  }
  if (M == 1 && !relu) {
    sr_rowdot(X, W, bias, Y, T, K, c.st);
    return 0;
  }
  hipLaunchKernelGGL(sr_gemm_xwT_ref_kernel, dim3((unsigned)((T * M + 255) / 256)), dim3(256), 0, c.st, X, W, bias, Y, T, K, M, relu);
  return 0;
}
// S[T, M] = (X[T, K] . W[M, K]^T + bias) + res: a Linear onto the residual stream, fused (the tiled GEMM only); false = the
// shape does not take it and the caller runs the Linear and the residual pass separately
bool gemm_xwT_res(const SrCall& c, const float* X, int64_t w, const float* bias, const float* res, float* S, int K, int M) {
  const int64_t T = c.p.T;
  const float* W = c.params + w;
  if (!(M >= 16 && M % 4 == 0 && vec_ok(X, S, K, M) && (((uintptr_t)res) & 15) == 0 && T * (K > M ? K : M) * 4 < ((int64_t)1 << 31)))
    return false;
  const ugemm::APlain a{X, T, K, K};
  const ugemm::EBiasRes e{S, bias, res, M};
  if (const SrPlan::SplitMat* sm = c.split(w, M, K)) {
    const ugemm::Dims dh{T, M, K, sm->ldK};
    const _Float16* hi = c.planes + sm->f_off;
    return ugemm::run_h3(dh, a, hi, hi + (int64_t)M * sm->ldK, e, c.st) == hipSuccess;
  }
  const ugemm::Dims d{T, M, K, K};
  return ugemm::run<true>(d, a, W, e, c.st) == hipSuccess;
}
// row-major  dX[T, K] = (accumulate ? dX : 0) + dY[T, M] . W[M, K], then zeroed where mask <= 0 (mask may be NULL)
int gemm_dyw(const SrCall& c, const float* dY, int64_t w, float* dX, const float* mask, int K, int M, int accumulate) {
  const int64_t T = c.p.T;
  const float* W = c.params + w;
  if (M % 4 == 0 && K >= 16 && vec_ok(dY, dX, K, K) && (mask == nullptr || ((uintptr_t)mask & 15) == 0) &&
      T * (K > M ? K : M) * 4 < ((int64_t)1 << 31)) {
    const ugemm::APlain a{dY, T, M, M};
    const ugemm::EStore e{dX, mask, K, accumulate};
    if (const SrPlan::SplitMat* sm = K >= 16 ? c.split(w, M, K) : nullptr) {  // the planes of W^T: [K][ldM], contraction over M
      const ugemm::Dims dh{T, K, M, sm->ldM};
      const _Float16* hi = c.planes + sm->t_off;
      return ugemm::run_h3(dh, a, hi, hi + (int64_t)K * sm->ldM, e, c.st) == hipSuccess ? 0 : ULTR_E_UNSUPPORTED;
    }
    const ugemm::Dims d{T, K, M, K};
    return ugemm::run<false>(d, a, W, e, c.st) == hipSuccess ? 0 : ULTR_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(sr_gemm_dyw_ref_kernel, dim3((unsigned)((T * K + 255) / 256)), dim3(256), 0, c.st, dY, W, dX, mask, T, K, M, accumulate);
  return 0;
}
// row-major  dW[M, K] = dY[T, M]^T . X[T, K] for the shapes sr_wgrad_kernel does not take: `wg_split` equal row chunks
// into partials, folded in canonical order
int gemm_dyTx(const SrCall& c, const float* dY, const float* X, float* dW, int K, int M) {
  const SrPlan& p = c.p;
  if (M == 1 && K <= 3 * p.maxw) {  // the scorer's weight row: weighted column sums
    sr_colsum_w(c, dY, X, K, dW);
    return 0;
  }
  const int S = p.wg_split;
  const int64_t rows = p.T / S;
  const int len = M * K;
  float* part = c.folds->scratch(c.ws + p.ws_wg, (int64_t)S * len);
  hipLaunchKernelGGL(sr_gemm_dyTx_ref_kernel, dim3((len + 255) / 256, S), dim3(256), 0, c.st, dY, X, part, rows, K, M);
  c.folds->add(part, (int64_t)len, S, len, dW, c.st);
  return 0;
}

// dW = dY^T X and (db != NULL) db = column sums of dY.  Aligned shapes go through sr_wgrad_kernel; the rest through
// the plain chunked kernel + the column-sum kernels.
int wgrad(const SrCall& c, const float* dY, const float* X, float* dW, float* db, int K, int M) {
  const SrPlan& p = c.p;
  const int64_t T = p.T;
  hipStream_t st = c.st;
  SrFoldQueue& q = *c.folds;
  const bool ok = M % 4 == 0 && K % 4 == 0 && (((uintptr_t)dY | (uintptr_t)X) & 15) == 0;
  if (!ok) {
    SR_CHECK(gemm_dyTx(c, dY, X, dW, K, M));
    if (db != nullptr) sr_colsum(c, dY, nullptr, nullptr, nullptr, M, 0, db);
    return 0;
  }
  // both kernels below leave S slabs [M * K | M] (dW | db): one fold where weight and bias are neighbours in the flat parameter
  // vector as they are in the slab, else one each
  const int64_t stride = (int64_t)M * K + M;
  const int len = M * K;
  auto fold_slabs = [&](const float* part, int S) {
    if (db == dW + len) {
      q.add(part, stride, S, len + M, dW, st);
    } else {
      q.add(part, stride, S, len, dW, st);
      if (db != nullptr) q.add(part + len, stride, S, M, db, st);
    }
  };
  {
    // square-ish products (d x d: 66 % matrix-core occupancy on the fp32 instruction) take the DNN's split-half weight-gradient
    // kernel: same slab layout, so the fold below is the same.  The thin ones (dff = 64 wide) run at their HBM floor already.
    int S2 = 0, rps2 = 0;
    if (c.planes != nullptr && c.knobs.wg_h3 != 0 && M >= 128 && K >= 128 && ultr_wgrad_h3_geometry(T, M, K, &S2, &rps2) &&
        (int64_t)S2 * stride <= p.wg_floats) {
      float* part2 = q.scratch(c.ws + p.ws_wg, (int64_t)S2 * stride);
      const int rc = ultr_wgrad_h3_plain(dY, X, T, M, K, part2, st);
      if (rc == 0) {
        fold_slabs(part2, S2);
        return 0;
      }
      if (rc != ULTR_E_UNSUPPORTED) return rc;
    }
  }
  int rps = 0;
  const int S = sr_wgrad_chunks(T, M, K, &rps);
  if ((int64_t)rps * (M > K ? M : K) * 4 >= ((int64_t)1 << 31)) return ULTR_E_UNSUPPORTED;
  const int nmb = (M + 63) / 64, nkb = (K + 63) / 64;
  float* part = q.scratch(c.ws + p.ws_wg, (int64_t)S * stride);
  const size_t lds = (size_t)(4 * 64 * 64 + 4 * 64) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(sr_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
      return ULTR_E_UNSUPPORTED;
    attr_set = true;
  }
  hipLaunchKernelGGL(sr_wgrad_kernel, dim3(nmb * nkb * S), dim3(256), lds, st, dY, X, T, M, K, nkb, S, rps, part);
  fold_slabs(part, S);
  return 0;
}

}  // namespace

void ultr_setrank_knobs_reload() { sr_knobs_load(); }

// bytes of `saved` (sr_make_plan) or of the scoring buffer (sr_make_score_plan): activations, planes, four floats with the range word
static int64_t sr_saved_bytes(const SrPlan& p) { return (p.sv_planes + (p.planes_halves + 1) / 2 + 4) * (int64_t)sizeof(float); }

extern "C" int32_t ultr_setrank_attn_path(const ultr_setrank_desc* c, int32_t list_size, int32_t backward) {
  SrPlan p;
  if (list_size <= 0 || !sr_make_plan(c, list_size, &p)) return ULTR_E_BADARG;
  const SrKnobs& k = sr_knobs();
  const SrAttnShape ash = {p.d, p.dh, p.H, p.att_f16, k.attn_long_min, p.stream_bwd};
  return sr_attn_path(ash, list_size, backward != 0, k.attn_h3 >= 1 && ((k.attn_mask >> 1) & 1) != 0);
}

// The route a plain step (dropout = 0) or a dropout step takes at batch x list_size: the plan and the route of the forward and the backward
// themselves (sr_make_plan, sr_route - no condition is restated here), under the knobs as last read, the descriptor's flags, the CU
// count the forward reads, and 16-byte aligned `saved`.  Launches nothing.
extern "C" int ultr_setrank_route(const ultr_setrank_desc* c, int32_t batch, int32_t list_size, int32_t dropout, ultr_setrank_route_info* out) {
  SrPlan p;
  if (out == nullptr || batch <= 0 || list_size <= 0 || !sr_make_plan(c, (int64_t)batch * list_size, &p)) return ULTR_E_BADARG;
  const SrKnobs& k = sr_knobs();
  const SrRoute rt = sr_route(p, k, sr_cu_count(), k.h3 && !p.no_h3, dropout != 0, true);
  memset(out, 0, sizeof(*out));
  out->embed = rt.embed; out->block = rt.block; out->head_rides = rt.head_rides; out->skip_out1 = rt.skip_out1;
  out->bwd_head = rt.bwd_head; out->bwd_blocks = rt.bwd_blocks; out->bwd_embed = rt.bwd_embed;
  out->rows_per_tile = rt.R; out->tiles = rt.tiles; out->workgroups = rt.nwg;
  out->block_rows = rt.block_R; out->embed_rows = rt.embed_R;
  out->wgrad_split = p.wg_split;
  return 0;
}

extern "C" int64_t ultr_setrank_param_count(const ultr_setrank_desc* c) {
  SrPlan p;
  return sr_make_plan(c, 0, &p) ? p.P : 0;
}
extern "C" int64_t ultr_setrank_saved_bytes(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_plan(c, n_rows, &p)) ? sr_saved_bytes(p) : 0;
}
extern "C" int64_t ultr_setrank_range_flag_offset(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_plan(c, n_rows, &p)) ? p.sv_flag : -1;
}
// the scoring entry's buffer (ultr_setrank_score): the live activations of sr_make_score_plan, the planes, the range word
extern "C" int64_t ultr_setrank_score_bytes(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_score_plan(c, n_rows, &p)) ? sr_saved_bytes(p) : 0;
}
extern "C" int64_t ultr_setrank_score_range_flag_offset(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_score_plan(c, n_rows, &p)) ? p.sv_flag : -1;
}
extern "C" int64_t ultr_setrank_workspace_bytes(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_plan(c, n_rows, &p)) ? (p.ws_total + 4) * (int64_t)sizeof(float) : 0;
}

namespace {

// ONE predicate for both directions of a step: a dropout step runs the separate launches (no sr_embed_fwd_kernel, no block kernels,
// no fused launches of ultr_sr_bwd.hip); NULL or rate == 0 is the plain step.  0: plain, 1: dropout (args filled), < 0: error
int sr_dropout_plan(const ultr_setrank_dropout* dr, int batch, int list_size, SrDropArgs* out) {
  if (dr == nullptr || dr->rate == 0.0f) return 0;
  const int rc = sr_drop_args(dr->rate, dr->seed, dr->step, dr->stream, batch, list_size, out);
  return rc != 0 ? rc : 1;
}
// floats of the backward's extra buffer: the masked branch gradient [T, d] and the bias column-sum partials of the 2 nl encoder sites
int64_t sr_dropout_ws_floats(const SrPlan& p) {
  return ((p.T * p.d + 3) & ~(int64_t)3) + (int64_t)2 * p.nl * ((sr_drop_parts(p.T) * p.d + 3) & ~(int64_t)3);
}

int setrank_forward(const ultr_setrank_desc* desc, const float* params, const float* features, int64_t n_docs,
                    const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* saved,
                    const ultr_setrank_dropout* dropout, void* stream, bool score = false, int64_t saved_bytes = 0) {
  if (!params || !docids || !scores || !saved || batch <= 0 || list_size <= 0 || n_docs < 0 || (n_docs > 0 && !features))
    return ULTR_E_BADARG;
  const int64_t T = (int64_t)batch * list_size;
  SrPlan p;
  if (!sr_make_plan_any(desc, T, &p, score)) return ULTR_E_BADARG;
  const int L = list_size;
  SrDropArgs da;
  const int drop_rc = sr_dropout_plan(dropout, batch, list_size, &da);
  if (drop_rc < 0) return drop_rc;
  const bool drop = drop_rc == 1;
  const SrAttnShape ash = {p.d, p.dh, p.H, p.att_f16, sr_knobs().attn_long_min, p.stream_bwd};
  SR_CHECK(sr_attn_supported(ash, L, 0));
  if (T > 0x7fffffff / 4) return ULTR_E_UNSUPPORTED;
  if (score && saved_bytes < sr_saved_bytes(p)) return ULTR_E_WORKSPACE;  // (ultr_setrank_score: the buffer comes with its size)
  hipStream_t st = (hipStream_t)stream;
  float* sv = (float*)saved;
  const int F = p.F, d = p.d, dff = p.dff;
  // a row of the plan nobody keeps (offset < 0, the scoring plan): NULL, and the kernel does not store it
  auto opt = [&](int64_t off) -> float* { return off < 0 ? nullptr : sv + off; };
  SrCall c = {p, params, nullptr, sr_knobs(), sr_cu_count(), sv, nullptr, st, nullptr};
  _Float16* planes = reinterpret_cast<_Float16*>(sv + p.sv_planes);
  const bool planes_on = c.knobs.h3 && !p.no_h3;
  const SrRoute rt = sr_route(p, c.knobs, c.cus, planes_on, drop, (((uintptr_t)sv | (uintptr_t)planes) & 15) == 0);
  // split-half planes of every weight matrix (the weights change with every update: rebuilt per forward, ~2 MB, one small launch)
  SR_CHECK((int)hipMemsetAsync(sv + p.sv_flag, 0, sizeof(uint32_t), st));  // this step's range word
  if (planes_on) {
    SrSplitTable tb;
    tb.n = p.n_split;
    int64_t maxe = 0;
    for (int k = 0; k < p.n_split; ++k) {
      tb.m[k] = p.split[k];
      const int64_t a = (int64_t)p.split[k].M * p.split[k].ldK, b = (int64_t)p.split[k].K * p.split[k].ldM;
      maxe = a > maxe ? a : maxe;
      maxe = b > maxe ? b : maxe;
    }
    hipLaunchKernelGGL(sr_split_planes_kernel, dim3((unsigned)((maxe + 255) / 256), (unsigned)(4 * p.n_split)), dim3(256), 0, st, tb, params, planes,
                       reinterpret_cast<uint32_t*>(sv + p.sv_flag));
    c.planes = planes;
  }
  // input LayerNorm on the gathered rows, then the embedding FFN (SetRank.py:134-135, 146)
  // (the features pointer is the forward's alone, so its tests sit here and not in the route: the kernel reads whole float4s of the
  // feature matrix through one buffer resource)
  if (rt.embed && n_docs > 0 && n_docs * (int64_t)F * 4 < ((int64_t)1 << 31) && ((uintptr_t)features & 15) == 0) {
    SR_CHECK(sr_embed_fwd(c, rt, features, docids, n_docs, (int)batch, L));  // one launch (sr_embed_fwd_kernel)
  } else {
    sr_ln_gather_fwd(features, docids, n_docs, (int)batch, L, T, F, params + p.g_in, params + p.b_in, opt(p.sv_xg), sv + p.sv_xn0,
                  opt(p.sv_mean_in), opt(p.sv_rstd_in), st);
    SR_CHECK(gemm_xwT(c, sv + p.sv_xn0, p.w1, params + p.b1, sv + p.sv_h0, F, dff, 1));
    SR_CHECK(gemm_xwT(c, sv + p.sv_h0, p.w2, params + p.b2, sv + p.sv_x[0], dff, d, 0));
  }
  if (drop) sr_drop_mask_launch(da, 0, sv + p.sv_x[0], sv + p.sv_x[0], nullptr, T, d, st);  // x0 = D(embedding): attention and the residual read it
  for (int l = 0; l < p.nl; ++l) {
    const SrLayer& y = p.lay[l];
    const float* x = sv + p.sv_x[l];
    SR_CHECK(sr_attn_forward(ash, x, batch, L, sv + p.sv_A[l], opt(p.sv_lse[l]), st));
    if (rt.block != SR_BLOCK_SEPARATE) {  // everything behind the attention in one launch
      SR_CHECK(sr_block_fwd(c, rt, l, scores));
      continue;
    }
    // A Wd^T lands in out1's buffer, then out1 = LN1(x + (A Wd^T + bd)) in place (s1 keeps the pre-norm sum)
    // the Linear's epilogue writes the pre-norm sum s1 = x + (A Wd^T + bd) straight into `saved` (one pass over [T, d] less on
    // each side of the LayerNorm); shapes the tiled GEMM does not take: Linear, then the residual pass
    if (drop) {  // o = D(dense(A)), f = D(ffn(out1)): the Linear without its bias, then dropout + residual + LayerNorm in one row pass
      SR_CHECK(gemm_xwT(c, sv + p.sv_A[l], y.wd, nullptr, sv + p.sv_out1[l], d, d, 0));
      sr_drop_ln_fwd_launch(da, 1 + 2 * l, x, sv + p.sv_out1[l], params + y.bd, T, d, params + y.g1, params + y.b1, sv + p.sv_s1[l],
                            sv + p.sv_out1[l], sv + p.sv_m1[l], sv + p.sv_r1[l], st);
      SR_CHECK(gemm_xwT(c, sv + p.sv_out1[l], y.wf1, params + y.bf1, sv + p.sv_f[l], d, dff, 1));
      SR_CHECK(gemm_xwT(c, sv + p.sv_f[l], y.wf2, nullptr, sv + p.sv_x[l + 1], dff, d, 0));
      sr_drop_ln_fwd_launch(da, 2 + 2 * l, sv + p.sv_out1[l], sv + p.sv_x[l + 1], params + y.bf2, T, d, params + y.g2, params + y.b2,
                            sv + p.sv_s2[l], sv + p.sv_x[l + 1], sv + p.sv_m2[l], sv + p.sv_r2[l], st);
      continue;
    }
    // the scoring plan runs both LayerNorms in place (s1 and out1 share a buffer, s2 and x_{l+1} do): where the row kernel itself forms
    // the pre-norm sum it then keeps none
    float* const s1_keep = p.sv_s1[l] == p.sv_out1[l] ? nullptr : sv + p.sv_s1[l];
    float* const s2_keep = p.sv_s2[l] == p.sv_x[l + 1] ? nullptr : sv + p.sv_s2[l];
    const bool ln_v4 = (d == 256 || d == 512 || d == 768 || d == 1024);
    if (ln_v4 && gemm_xwT_res(c, sv + p.sv_A[l], y.wd, params + y.bd, x, sv + p.sv_s1[l], d, d)) {
      sr_ln_residual_fwd(sv + p.sv_s1[l], nullptr, nullptr, T, d, params + y.g1, params + y.b1, nullptr, sv + p.sv_out1[l],
                      opt(p.sv_m1[l]), opt(p.sv_r1[l]), (int)batch, L, st);
    } else {
      SR_CHECK(gemm_xwT(c, sv + p.sv_A[l], y.wd, nullptr, sv + p.sv_out1[l], d, d, 0));
      sr_ln_residual_fwd(x, sv + p.sv_out1[l], params + y.bd, T, d, params + y.g1, params + y.b1, s1_keep, sv + p.sv_out1[l],
                      opt(p.sv_m1[l]), opt(p.sv_r1[l]), (int)batch, L, st);
    }
    SR_CHECK(gemm_xwT(c, sv + p.sv_out1[l], y.wf1, params + y.bf1, sv + p.sv_f[l], d, dff, 1));
    if (ln_v4 && gemm_xwT_res(c, sv + p.sv_f[l], y.wf2, params + y.bf2, sv + p.sv_out1[l], sv + p.sv_s2[l], dff, d)) {
      sr_ln_residual_fwd(sv + p.sv_s2[l], nullptr, nullptr, T, d, params + y.g2, params + y.b2, nullptr, sv + p.sv_x[l + 1],
                      opt(p.sv_m2[l]), opt(p.sv_r2[l]), (int)batch, L, st);
    } else {
      SR_CHECK(gemm_xwT(c, sv + p.sv_f[l], y.wf2, nullptr, sv + p.sv_x[l + 1], dff, d, 0));
      sr_ln_residual_fwd(sv + p.sv_out1[l], sv + p.sv_x[l + 1], params + y.bf2, T, d, params + y.g2, params + y.b2, s2_keep,
                      sv + p.sv_x[l + 1], opt(p.sv_m2[l]), opt(p.sv_r2[l]), (int)batch, L, st);
    }
  }
  // output FFN (SetRank.py:136, 153)
  if (!rt.head_rides) {
    SR_CHECK(gemm_xwT(c, sv + p.sv_x[p.nl], p.wo1, params + p.bo1, sv + p.sv_oh, d, dff, 1));
    SR_CHECK(gemm_xwT(c, sv + p.sv_oh, p.wo2, params + p.bo2, scores, dff, 1, 0));
  }
  return (int)hipGetLastError();
}

int setrank_backward(const ultr_setrank_desc* desc, const float* params, int32_t batch, int32_t list_size,
                     const void* saved, const float* dscores, const void* loss_ws, int32_t n_loss_parts, void* ws_,
                     float* grads, const ultr_setrank_dropout* dropout, void* stream) {
  if (!params || !saved || !dscores || !ws_ || !grads || batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  const int64_t T = (int64_t)batch * list_size;
  SrPlan p;
  if (!sr_make_plan(desc, T, &p)) return ULTR_E_BADARG;
  const int L = list_size;
  SrDropArgs da;
  const int drop_rc = sr_dropout_plan(dropout, batch, list_size, &da);
  if (drop_rc < 0) return drop_rc;
  const bool drop = drop_rc == 1;
  float* DM = nullptr;     // the masked branch gradient of the site at hand [T, d]
  float* dpart = nullptr;  // its bias column-sum partials, one piece per encoder site (the folds run at the end)
  int64_t dpart_floats = 0;
  if (drop) {
    if (dropout->scratch == nullptr || ((uintptr_t)dropout->scratch & 15) != 0 ||
        dropout->scratch_bytes < sr_dropout_ws_floats(p) * (int64_t)sizeof(float))
      return ULTR_E_WORKSPACE;
    DM = (float*)dropout->scratch;
    dpart = DM + ((T * p.d + 3) & ~(int64_t)3);
    dpart_floats = (sr_drop_parts(T) * p.d + 3) & ~(int64_t)3;
  }
  const SrAttnShape ash = {p.d, p.dh, p.H, p.att_f16, sr_knobs().attn_long_min, p.stream_bwd};
  SR_CHECK(sr_attn_supported(ash, L, 1));
  hipStream_t st = (hipStream_t)stream;
  const float* sv = (const float*)saved;
  float* ws = (float*)ws_;
  float* G0 = ws + p.ws_g[0];
  float* G1 = ws + p.ws_g[1];
  float* G2 = ws + p.ws_g[2];
  float* attn_t = p.ws_attn_t >= 0 ? ws + p.ws_attn_t : nullptr;  // the streaming attention backward's t = dA . A
  const int F = p.F, d = p.d, dff = p.dff;
  SrFoldQueue folds(ws + p.ws_arena, p.arena_floats);  // every fold below is queued; ONE launch at the end
  SrCall c = {p, params, nullptr, sr_knobs(), sr_cu_count(), const_cast<float*>(sv), ws, st, &folds};
  if (c.knobs.h3 && !p.no_h3) c.planes = reinterpret_cast<const _Float16*>(sv + p.sv_planes);  // built by this step's forward
  // the route this step's forward took as well (same inputs): it left out1 unwritten exactly where rt.bwd_blocks recomputes it.  The
  // fused launches (ultr_sr_bwd.hip) read the transposed fragment copies built by that forward and leave per-workgroup partials in
  // arena pieces the plan sized: a missing piece is an error (ULTR_E_WORKSPACE), never a change of path
  const SrRoute rt = sr_route(p, c.knobs, c.cus, c.planes != nullptr, drop, (((uintptr_t)sv | (uintptr_t)c.planes) & 15) == 0);
  // ULTR_SR_ATTN_H3 and its mask (bit 2 layer + 1: this layer's backward) allow the split-half attention backward kernel
  auto attn_split_half = [&](int layer) { return c.knobs.attn_h3 >= 1 && ((c.knobs.attn_mask >> (2 * layer + 1)) & 1) != 0; };
  // ---- output FFN:  s = oh wo2^T + bo2,  oh = relu(x_nl Wo1^T + bo1) ----------------------------------------------
  if (rt.bwd_head) {
    const int64_t sh = ((int64_t)dff * d + 2 * dff + 2 + 3) & ~(int64_t)3;  // (whole float4s: sr_fold_all_kernel's vector form)
    float* ph = folds.piece(rt.nwg * sh);
    if (ph == nullptr) return ULTR_E_WORKSPACE;
    SrBwdHeadArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.R = rt.R; ha.d = d; ha.dff = dff; ha.ntiles = rt.tiles; ha.T = T;
    ha.dx = p.ws_g[0]; ha.x = p.sv_x[p.nl]; ha.oh = p.sv_oh; ha.wo2 = p.wo2; ha.gto1 = c.split(p.wo1, dff, d)->gt_off;
    ha.part = ph - ws; ha.part_stride = sh;
    SR_CHECK(sr_bwd_head_launch(ha, rt.nwg, params, c.planes, sv, dscores, ws, st));  // G0 = d x_nl
    folds.add(ph, sh, rt.nwg, dff * d + 2 * dff + 1, grads + p.wo1, st);              // d Wo1 | d bo1 | d wo2 | d bo2
  } else {
    if (dff <= 256) {  // one pass: G1 = d oh [T, dff] (ReLU mask fused), d wo2 | d bo2 partials
      sr_head_bwd(c, dscores, sv + p.sv_oh, params + p.wo2, dff, G1, grads + p.wo2);
    } else {
      SR_CHECK(gemm_dyTx(c, dscores, sv + p.sv_oh, grads + p.wo2, dff, 1));
      sr_colsum(c, dscores, nullptr, nullptr, nullptr, 1, 0, grads + p.bo2);
      SR_CHECK(gemm_dyw(c, dscores, p.wo2, G1, sv + p.sv_oh, dff, 1, 0));  // G1 = d oh  [T, dff], ReLU mask fused
    }
    SR_CHECK(wgrad(c, G1, sv + p.sv_x[p.nl], grads + p.wo1, grads + p.bo1, d, dff));
    SR_CHECK(gemm_dyw(c, G1, p.wo1, G0, nullptr, d, dff, 0));     // G0 = d x_nl  [T, d]
  }
  for (int l = p.nl - 1; l >= 0; --l) {
    const SrLayer& y = p.lay[l];
    if (rt.bwd_blocks) {
      const int64_t sa = (int64_t)d * dff + 3 * d, sb = (int64_t)dff * d + dff + 3 * d;
      float* pa = folds.piece(rt.nwg * sa);
      float* pb = folds.piece(rt.nwg * sb);
      if (pa == nullptr || pb == nullptr) return ULTR_E_WORKSPACE;
      SrBwdFfnArgs fa;
      memset(&fa, 0, sizeof(fa));
      fa.R = rt.R; fa.d = d; fa.dff = dff; fa.ntiles = rt.tiles; fa.T = T;
      fa.dy = p.ws_g[0]; fa.dF = p.ws_g[1]; fa.dx = p.ws_g[2];
      fa.s = p.sv_s2[l]; fa.mean = p.sv_m2[l]; fa.rstd = p.sv_r2[l]; fa.f = p.sv_f[l];
      fa.gamma = y.g2; fa.gt2 = c.split(y.wf2, d, dff)->gt_off; fa.gt1 = c.split(y.wf1, dff, d)->gt_off;
      fa.part = pa - ws; fa.part_stride = sa;
      SR_CHECK(sr_bwd_ffn_launch(fa, rt.nwg, params, c.planes, sv, ws, st));  // G1 = d f, G2 = d out1
      folds.add(pa, sa, rt.nwg, d * dff + d, grads + y.wf2, st);                 // d Wf2 | d bf2
      folds.add(pa + (int64_t)d * dff + d, sa, rt.nwg, 2 * d, grads + y.g2, st);  // d g2 | d b2
      SrBwdProjArgs pr;
      memset(&pr, 0, sizeof(pr));
      pr.R = rt.R; pr.d = d; pr.dff = dff; pr.ntiles = rt.tiles; pr.T = T;
      pr.dy = p.ws_g[2]; pr.dF = p.ws_g[1]; pr.ds = p.ws_g[0]; pr.dx = p.ws_g[2];
      pr.s = p.sv_s1[l]; pr.mean = p.sv_m1[l]; pr.rstd = p.sv_r1[l];
      pr.gamma = y.g1; pr.beta = y.b1; pr.gtd = c.split(y.wd, d, d)->gt_off;
      pr.part = pb - ws; pr.part_stride = sb;
      SR_CHECK(sr_bwd_proj_launch(pr, rt.nwg, params, c.planes, sv, ws, st));  // G0 = d s1 (= d x_l through the residual), G2 = d A
      folds.add(pb, sb, rt.nwg, dff * d + dff, grads + y.wf1, st);                      // d Wf1 | d bf1
      folds.add(pb + (int64_t)dff * d + dff, sb, rt.nwg, d, grads + y.bd, st);          // d bd
      folds.add(pb + (int64_t)dff * d + dff + d, sb, rt.nwg, 2 * d, grads + y.g1, st);  // d g1 | d b1
      SR_CHECK(wgrad(c, G0, sv + p.sv_A[l], grads + y.wd, nullptr, d, d));
      // G0 += attention path -> d x_l
      SR_CHECK(sr_attn_backward(ash, attn_split_half(l), sv + p.sv_x[l], G2, sv + p.sv_A[l], sv + p.sv_lse[l], batch, L, G0, attn_t, st));
      continue;
    }
    // the separate launches: they read out1, which this step's forward wrote (rt.skip_out1 implies rt.bwd_blocks)
    // a dropout site: the branch gradient d(b + bias) = keep * scale * ds goes to DM with its column sums (the bias gradient); the
    // residual keeps the unmasked ds
    auto masked_branch = [&](int site, const float* ds, float* dst_bias) {
      float* part = dpart + (int64_t)(site - 1) * dpart_floats;
      sr_drop_mask_launch(da, site, ds, DM, part, T, d, st);
      folds.add(part, (int64_t)d, (int)sr_drop_parts(T), d, dst_bias, st, /*own_buffer=*/true);
    };
    // x_{l+1} = LN2(s2),  s2 = out1 + ffn
    if (d <= 1024) {  // g2 | b2, G2 = d s2 = d out1 (residual) = d ffn, bf2: one pass
      SR_CHECK(sr_ln_bwd_cs(c, G0, sv + p.sv_s2[l], sv + p.sv_m2[l], sv + p.sv_r2[l], params + y.g2, d, G2, grads + y.g2,
                         drop ? nullptr : grads + y.bf2));
    } else {
      sr_colsum_ln(c, G0, sv + p.sv_s2[l], sv + p.sv_m2[l], sv + p.sv_r2[l], d, grads + y.g2);
      sr_ln_bwd_rows(c, G0, sv + p.sv_s2[l], sv + p.sv_m2[l], sv + p.sv_r2[l], params + y.g2, d, G2);
      if (!drop) sr_colsum(c, G2, nullptr, nullptr, nullptr, d, 0, grads + y.bf2);
    }
    if (drop) masked_branch(2 + 2 * l, G2, grads + y.bf2);
    const float* dffn = drop ? DM : G2;  // d (f Wf2^T + bf2)
    SR_CHECK(wgrad(c, dffn, sv + p.sv_f[l], grads + y.wf2, nullptr, dff, d));
    SR_CHECK(gemm_dyw(c, dffn, y.wf2, G1, sv + p.sv_f[l], dff, d, 0));  // G1 = d f  [T, dff], ReLU mask fused
    SR_CHECK(wgrad(c, G1, sv + p.sv_out1[l], grads + y.wf1, grads + y.bf1, d, dff));
    SR_CHECK(gemm_dyw(c, G1, y.wf1, G2, nullptr, d, dff, 1));   // G2 = d out1 (both paths): accumulated
    // out1 = LN1(s1),  s1 = x_l + o
    if (d <= 1024) {  // g1 | b1, G0 = d s1 = d x_l (residual) = d o, bd
      SR_CHECK(sr_ln_bwd_cs(c, G2, sv + p.sv_s1[l], sv + p.sv_m1[l], sv + p.sv_r1[l], params + y.g1, d, G0, grads + y.g1,
                         drop ? nullptr : grads + y.bd));
    } else {
      sr_colsum_ln(c, G2, sv + p.sv_s1[l], sv + p.sv_m1[l], sv + p.sv_r1[l], d, grads + y.g1);
      sr_ln_bwd_rows(c, G2, sv + p.sv_s1[l], sv + p.sv_m1[l], sv + p.sv_r1[l], params + y.g1, d, G0);
      if (!drop) sr_colsum(c, G0, nullptr, nullptr, nullptr, d, 0, grads + y.bd);
    }
    if (drop) masked_branch(1 + 2 * l, G0, grads + y.bd);
    const float* dproj = drop ? DM : G0;  // d (A Wd^T + bd)
    SR_CHECK(wgrad(c, dproj, sv + p.sv_A[l], grads + y.wd, nullptr, d, d));
    SR_CHECK(gemm_dyw(c, dproj, y.wd, G1, nullptr, d, d, 0));      // G1 = d A  [T, d]
    // G0 += attention path -> d x_l
    SR_CHECK(sr_attn_backward(ash, attn_split_half(l), sv + p.sv_x[l], G1, sv + p.sv_A[l], sv + p.sv_lse[l], batch, L, G0, attn_t, st));
  }
  // ---- embedding FFN and the input LayerNorm's parameters -------------------------------------------------------------
  if (drop) sr_drop_mask_launch(da, 0, G0, G0, nullptr, T, d, st);  // x0 has no residual: d embedding = D'(d x0) in place; wgrad sums d b2
  if (rt.bwd_embed) {
    const int64_t se = (int64_t)2 * F + (int64_t)dff * F + dff + (int64_t)d * dff + d;
    float* pe = folds.piece(rt.nwg * se);
    if (pe == nullptr) return ULTR_E_WORKSPACE;
    SrBwdEmbedArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.R = rt.R; ea.d = d; ea.dff = dff; ea.F = F; ea.ntiles = rt.tiles; ea.T = T;
    ea.dy = p.ws_g[0]; ea.h0 = p.sv_h0; ea.xg = p.sv_xg; ea.mean = p.sv_mean_in; ea.rstd = p.sv_rstd_in;
    ea.g_in = p.g_in; ea.b_in = p.b_in; ea.gt2 = c.split(p.w2, d, dff)->gt_off; ea.gt1 = c.split(p.w1, dff, F)->gt_off;
    ea.part = pe - ws; ea.part_stride = se;
    SR_CHECK(sr_bwd_embed_launch(ea, rt.nwg, params, c.planes, sv, ws, st));
    folds.add(pe, se, rt.nwg, (int)se, grads + p.g_in, st);  // d g_in | d b_in | d W1 | d b1 | d W2 | d b2
  } else {
    SR_CHECK(wgrad(c, G0, sv + p.sv_h0, grads + p.w2, grads + p.b2, dff, d));
    SR_CHECK(gemm_dyw(c, G0, p.w2, G1, sv + p.sv_h0, dff, d, 0));  // ReLU mask fused
    SR_CHECK(wgrad(c, G1, sv + p.sv_xn0, grads + p.w1, grads + p.b1, F, dff));
    SR_CHECK(gemm_dyw(c, G1, p.w1, G2, nullptr, F, dff, 0));      // G2 = d xn0  [T, F]
    sr_colsum_ln(c, G2, sv + p.sv_xg, sv + p.sv_mean_in, sv + p.sv_rstd_in, F, grads + p.g_in);  // g_in | b_in
  }
  // ---- step tail: fold the loss partials behind the gradient ----------------------------------------------------------
  if (loss_ws != nullptr && n_loss_parts > 0) {
    const int tail = (int)ultr_tail_len(list_size);
    folds.add((const float*)loss_ws, (int64_t)tail, (int)n_loss_parts, tail, grads + p.P, st, /*own_buffer=*/true);
  }
  folds.flush(st);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int ultr_setrank_forward(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                                    const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* saved,
                                    void* stream) {
  return setrank_forward(c, params, features, n_docs, docids, batch, list_size, scores, saved, nullptr, stream);
}
extern "C" int ultr_setrank_backward(const ultr_setrank_desc* c, const float* params, int32_t batch, int32_t list_size,
                                     const void* saved, const float* dscores, const void* loss_ws, int32_t n_loss_parts, void* ws_,
                                     float* grads, void* stream) {
  return setrank_backward(c, params, batch, list_size, saved, dscores, loss_ws, n_loss_parts, ws_, grads, nullptr, stream);
}
extern "C" int64_t ultr_setrank_dropout_workspace_bytes(const ultr_setrank_desc* c, int64_t n_rows) {
  SrPlan p;
  return (n_rows >= 0 && sr_make_plan(c, n_rows, &p)) ? sr_dropout_ws_floats(p) * (int64_t)sizeof(float) : 0;
}
// The evaluation forward: the bits of ultr_setrank_forward in `scores`, no record for a backward - `work` (ultr_setrank_score_bytes) holds
// what the launches hand to each other, the planes and the range word (ultr_setrank_score_range_flag_offset).  Same driver, same route,
// the scoring plan (sr_make_score_plan, ultr_sr_plan.h).
extern "C" int ultr_setrank_score(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                                  const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* work, int64_t work_bytes,
                                  void* stream) {
  return setrank_forward(c, params, features, n_docs, docids, batch, list_size, scores, work, nullptr, stream, true, work_bytes);
}
extern "C" int ultr_setrank_forward_dropout(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                                            const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* saved,
                                            const ultr_setrank_dropout* dropout, void* stream) {
  return setrank_forward(c, params, features, n_docs, docids, batch, list_size, scores, saved, dropout, stream);
}
extern "C" int ultr_setrank_backward_dropout(const ultr_setrank_desc* c, const float* params, int32_t batch, int32_t list_size,
                                             const void* saved, const float* dscores, const void* loss_ws, int32_t n_loss_parts,
                                             void* ws_, float* grads, const ultr_setrank_dropout* dropout, void* stream) {
  return setrank_backward(c, params, batch, list_size, saved, dscores, loss_ws, n_loss_parts, ws_, grads, dropout, stream);
}
