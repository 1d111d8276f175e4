// ultr_sr_block.hip - SetRank forward, the fused kernels of round 5 and the launchers of the route's fused forward launches:
//   sr_block_fwd_kernel  everything of an encoder block behind the attention (+ the output FFN on the last block), one launch
//   sr_embed_fwd_kernel  feature gather + input LayerNorm + embedding FFN, one launch
// Two 8-wave workgroups per compute unit, each owning R <= 32 token rows through the whole chain.  For d_model 256 / dff 64 the
// persistent form of the block kernel (sr_fwd_block_kernel, ultr_sr_fwd.hip: round 6) takes over; sr_block_fwd() below launches
// whichever the step's route (SrRoute, ultr_sr_plan.h) names.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_h3.h"
#include "ultr_plan.h"
#include "ultr_sr_plan.h"
#ifdef ULTR_TRACE
// phase tracing (tools/trace_sr_block.py): sr_block_fwd_kernel stamps slots 20 .. 30 of the GEMM kernels' trace array, which lives in
// ultr_setrank.hip's code object (ultr_gemm_trace_arm / _read) - so the kernel gets its address as an argument
unsigned long long* sr_gemm_trace_slots();
#define SR_BLOCK_STAMP(slot)                                                                                                              \
  do {                                                                                                                                    \
    if (threadIdx.x == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 64 && a.trace && a.trace[(blockIdx.x >> 3) * 32 + 31] == 0ull)   \
      a.trace[(blockIdx.x >> 3) * 32 + (slot)] = __builtin_amdgcn_s_memtime();                                                            \
  } while (0)
#else
#define SR_BLOCK_STAMP(slot) \
  do {                       \
  } while (0)
#endif

namespace {

constexpr int NW = 8;  // waves per workgroup

// ---------------------------------------------------------------------------------------------------------
// Everything of an encoder block behind the attention, one launch (round 5): the wide-tile geometry of dnn_fwdw_kernel
// ---------------------------------------------------------------------------------------------------------
//   s1 = x + (A Wd^T + bd),  out1 = LN1(s1),  f = relu(out1 Wf1^T + bf1),  s2 = out1 + (f Wf2^T + bf2),  x' = LN2(s2)
// (SetRank.py:92-111) were two Linear + residual GEMMs, a Linear + ReLU GEMM and two LayerNorm launches: 1.1 GB of HBM traffic per
// block at config 5 for five tensors the backward wants saved (s1, out1, f, s2, x': 0.45 GB) and two it has to read (A, x: 0.2 GB).
// Here a workgroup of eight waves owns R <= 32 token rows through all of it: the three products run on split-half fragment
// copies of the weights (384 KB per block at config 5, streamed once per workgroup; built next to the GEMM planes by
// sr_split_planes_kernel), in the d-wide products wave = one 32-column chunk x the two row tiles over the WHOLE contraction (no
// partial sums; the kernel once had a 16-wave form whose second group of eight took two more row tiles - `g`, always 0 now), the
// dff-wide product splits (row tile, chunk, slice of the contraction) over the waves; activations live in three LDS buffers; every
// saved tensor leaves through a buffer resource clipped to the rows that exist.
struct SrBlockArgs {
  int R, d, dff;
  int64_t T;
  int64_t bd, bf1, bf2, g1, b1, g2, b2;                  // float offsets into the parameter vector
  int64_t gd, gf1, gf2;                                  // HALF offsets of the fragment-major copies of Wd, Wf1, Wf2 from the planes
  int64_t A, x, s1, m1, r1, out1, f, s2, m2, r2, xn;     // float offsets into `saved`; s1 .. r2 (not xn) < 0: not stored (the scoring forward)
  int p0, p1, p2, pv;                                    // float offsets into dynamic LDS
  // the last block also runs the output FFN (SetRank.py:136, 153): oh = relu(x' Wo1^T + bo1), score = oh . wo2 + bo2
  int head;
  int skip_out1;  // the backward recomputes out1 from s1 (sr_bwd_proj_kernel): the forward does not write it (105 MB per block at config 5)
  int64_t go1, bo1, wo2, bo2, oh;                        // fragment copy of Wo1 (halves), parameter offsets, saved oh (< 0: not stored)
#ifdef ULTR_TRACE
  unsigned long long* trace;
#endif
};

__device__ __forceinline__ float2 buf_ld2(const Src& s, unsigned byte_off) {
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(s.rs, byte_off, 0, 0);
  return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
}

// eight waves, up to 32 rows and 80 KB of LDS: two workgroups per CU, each other's memory waits and phases overlapping
__global__ __launch_bounds__(NW * 64) void sr_block_fwd_kernel(SrBlockArgs a, const float* __restrict__ params,
                                                            const _Float16* __restrict__ planes, float* __restrict__ sv,
                                                            float* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = NW * 64, RT = 4;  // a wave owns rows wave + NW q, q < 4, in the row-wise phases
  const int R = a.R, d = a.d, dff = a.dff;
  const int ld = d + 8, ldf = dff + 8;  // row strides: floats of an fp32 row = halves of a plane row
  float* P0 = smem + a.p0;   // planes of the current d-wide A operand (attention output, then out1)
  float* P1 = smem + a.p1;   // fp32 rows: s1 -> out1 -> s2
  float* P2 = smem + a.p2;   // planes of f
  float* PV = smem + a.pv;   // bd | g1 | b1 | bf2 | g2 | b2 | bf1 | bo1 | wo2 | bo2 (+ 3 pad)
  float* OS = PV + 6 * d + 3 * dff + 4;  // [64] row scales of the d-wide operand, [64] of f
  const int tid = threadIdx.x, lane_id = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n0 = (int64_t)blockIdx.x * R;
  const int vr = (int)((a.T - n0) < R ? (a.T - n0) : R);
  const float* pbd = PV, *pg1 = PV + d, *pb1 = PV + 2 * d, *pbf2 = PV + 3 * d, *pg2 = PV + 4 * d, *pb2 = PV + 5 * d, *pbf1 = PV + 6 * d;
  const float invd = 1.0f / (float)d;

  SR_BLOCK_STAMP(20);
  // the residual rows of x in the accumulator layout of the first product (wave = chunk x pair of row tiles): requested FIRST - they
  // are the only HBM operand of that product's epilogue and land while the prologue and the product run (measured against a drained
  // request: no difference, 2.57 - 2.59 ms either way - the phases wait for each other, not for HBM)
  float2 xres[2][4];
  {
    const int ch = wave & 7, g = wave >> 3, i = lane_id & 15, q = lane_id >> 4;
    const Src xs = make_src(sv + a.x + n0 * d, (int64_t)vr * d);
    const int col = 32 * ch + 2 * i;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        xres[t][r] = buf_ld2(xs, ch < (d >> 5) ? (unsigned)((16 * (2 * g + t) + 4 * q + r) * d + col) * 4u : ULTR_OOB);
  }
  // ---- prologue: parameter vectors to LDS; the attention rows as two fp16 planes scaled per row -------------------------------
  {
    const int lane = lane_id;
    for (int e = tid; e < 6 * d + dff; e += NT) {
      const int v = e / d;  // 0 .. 5: the d-long vectors; 6 ..: bf1
      const int64_t src = v == 0 ? a.bd : v == 1 ? a.g1 : v == 2 ? a.b1 : v == 3 ? a.bf2 : v == 4 ? a.g2 : v == 5 ? a.b2 : a.bf1;
      PV[e] = params[src + (v < 6 ? e - v * d : e - 6 * d)];
    }
    if (a.head)
      for (int e = tid; e < 2 * dff + 1; e += NT)
        PV[6 * d + dff + e] = params[e < dff ? a.bo1 + e : e < 2 * dff ? a.wo2 + (e - dff) : a.bo2];
    const Src as = make_src(sv + a.A + n0 * d, (int64_t)vr * d);
    const int c = 4 * lane;
    float4 av[RT];
    float am[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q;
      av[q] = buf_ld4(as, c < d ? (unsigned)(r * d + c) * 4u : ULTR_OOB);
      am[q] = fmaxf(fmaxf(fabsf(av[q].x), fabsf(av[q].y)), fmaxf(fabsf(av[q].z), fabsf(av[q].w)));
    }
    wave_max_n<RT>(am);
    _Float16* AH = reinterpret_cast<_Float16*>(P0);
    _Float16* AL = AH + (R + 1) * ld;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      float rs, inv;
      fb_h3_scale(am[q], rs, inv);
      if (c < d) {
        fbh4 hi, lo;
        fb_h3_split4(av[q], rs, hi, lo);
        *reinterpret_cast<fbh4*>(AH + rc * ld + c) = hi;
        *reinterpret_cast<fbh4*>(AL + rc * ld + c) = lo;
      }
      if (lane == 0) OS[r] = inv * (1.0f / ULTR_H3_WSCALE);
    }
  }
  lds_barrier();

  // a d-wide product: wave = (32-column chunk, pair of row tiles); Y = (planes . W) x row scale + bias + residual -> P1 + saved
  auto product_d = [&](const float* Ap, int lda, int nks, int64_t gw, int Kw, const float* bias, const float* os, bool res_lds,
                       int64_t out_off) {
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int nch = d >> 5;
    const int ch = wave & 7, g = wave >> 3;
    const bool has = ch < nch;
    const int i = lane & 15, q = lane >> 4;
    const _Float16* AH = reinterpret_cast<const _Float16*>(Ap);
    const int lo_off = (R + 1) * lda;
    const _Float16* pa[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 16 * (2 * g + t) + i;
      pa[t] = AH + (row < R ? row : R) * lda + 8 * q;
    }
    const Src Wh = make_src(reinterpret_cast<const float*>(planes + gw), (int64_t)Kw * d / 2 * 2);
    const int col = 32 * ch + 2 * i;
    PipeH3W<2, 2> ph;
    ph.begin(Wh, ch, nks, 0, nks, has, lane);
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) acc[t][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ph.run(pa, lo_off, Wh, has ? nks : 0, acc);
    if (has) {
      const Dst dout = make_dst_opt(sv, out_off, n0 * d, (int64_t)vr * d);
      const float2 bv = *reinterpret_cast<const float2*>(bias + col);
      const unsigned gv = (unsigned)(4 * q * d + 2 * i) * 4u;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 o4 = ld4(os + 16 * (2 * g + t) + 4 * q);
        const float o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * (2 * g + t) + 4 * q + r;
          const int rc = row < R ? row : R;
          float2* dst = reinterpret_cast<float2*>(P1 + rc * ld + col);
          const float2 rv = res_lds ? *dst : xres[t][r];
          const float2 y = make_float2(rv.x + (acc[t][0][r] * o[r] + bv.x), rv.y + (acc[t][1][r] * o[r] + bv.y));
          *dst = y;
          buf_st2(dout, gv, (unsigned)((16 * (2 * g + t) + r) * d + 32 * ch) * 4u, y);
        }
      }
    }
  };
  // LayerNorm of the rows in P1 (a wave owns rows wave + NW q): statistics and the output to `saved`; planes: the output also stays
  // in P1 (the residual of the next sum) and goes to P0 as the two fp16 planes of the next product's operand
  auto layer_norm = [&](const float* gam, const float* bet, int64_t mean_off, int64_t rstd_off, int64_t out_off, bool to_planes, bool store_out = true) {
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int c = 4 * lane;
    const bool cok = c < d;
    float4 v[RT];
    float s[RT], qv[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q;
      v[q] = cok ? ld4(P1 + (r < R ? r : R) * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      s[q] = (v[q].x + v[q].y) + (v[q].z + v[q].w);
    }
    wave_sum_n<RT>(s);
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      s[q] *= invd;
      if (cok) {
        v[q].x -= s[q]; v[q].y -= s[q]; v[q].z -= s[q]; v[q].w -= s[q];
      }
      qv[q] = (v[q].x * v[q].x + v[q].y * v[q].y) + (v[q].z * v[q].z + v[q].w * v[q].w);
    }
    wave_sum_n<RT>(qv);
    const Dst dmean = make_dst_opt(sv, mean_off, n0, vr), drstd = make_dst_opt(sv, rstd_off, n0, vr);
    const Dst dout = make_dst_opt(sv, out_off, n0 * d, (int64_t)vr * d);
    const unsigned l0 = lane == 0 ? 0u : ULTR_OOB;
    const float4 g4 = cok ? ld4(gam + c) : make_float4(0.f, 0.f, 0.f, 0.f), b4 = cok ? ld4(bet + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float am[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q;
      const float rstd = 1.0f / sqrtf(qv[q] * invd + SR_EPS);
      v[q] = make_float4(v[q].x * rstd * g4.x + b4.x, v[q].y * rstd * g4.y + b4.y, v[q].z * rstd * g4.z + b4.z, v[q].w * rstd * g4.w + b4.w);
      buf_st4(dout, (cok && store_out) ? (unsigned)c * 4u : ULTR_OOB, (unsigned)(r * d) * 4u, v[q]);
      buf_st1(dmean, l0, (unsigned)r * 4u, s[q]);
      buf_st1(drstd, l0, (unsigned)r * 4u, rstd);
      am[q] = fmaxf(fmaxf(fabsf(v[q].x), fabsf(v[q].y)), fmaxf(fabsf(v[q].z), fabsf(v[q].w)));
    }
    if (to_planes) {
      wave_max_n<RT>(am);
      _Float16* AH = reinterpret_cast<_Float16*>(P0);
      _Float16* AL = AH + (R + 1) * ld;
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        const int r = wave + NW * q, rc = r < R ? r : R;
        float rs, inv;
        fb_h3_scale(am[q], rs, inv);
        if (cok) {
          st4(P1 + rc * ld + c, v[q]);
          fbh4 hi, lo;
          fb_h3_split4(v[q], rs, hi, lo);
          *reinterpret_cast<fbh4*>(AH + rc * ld + c) = hi;
          *reinterpret_cast<fbh4*>(AL + rc * ld + c) = lo;
        }
        if (lane == 0) OS[r] = inv * (1.0f / ULTR_H3_WSCALE);
      }
    }
  };

  // a dff-wide product with ReLU (dff = 32 / 64 / 128: 1 / 2 / 4 chunks of 32 columns): wave = (row tile, chunk, slice of the contraction),
  // the partial tiles summed slice by slice into P2 as fp32 rows; then every wave finishes its own rows (wave + NW q): bias, ReLU, the
  // row to `saved`, and either the two fp16 planes scaled by the row maximum (the block's f) or the dot product with a vector (the scorer).
  // (The first version gave a whole row tile to ONE wave - the row maximum a 16-lane reduction - and two of eight waves did all of
  // it: ~50 us of the launch's 190.)
  auto product_f = [&](int64_t gw, const float* bias, int64_t out_off, const float* wdot, float bdot) {
    float* F32 = P2;
    {
      int lane = lane_id;
      asm volatile("" : "+v"(lane));
      const int i = lane & 15, q = lane >> 4, nks = d >> 5, nchf = dff >> 5, ksplit = 4 / nchf;
      const int rt = wave >> 2;
      int ch = wave & 3, ks = 0;
      while (ch >= nchf) { ch -= nchf; ++ks; }
      const int len = (nks + ksplit - 1) / ksplit, k0 = ks * len;
      const int cnt = k0 >= nks ? 0 : (k0 + len < nks ? len : nks - k0);
      const _Float16* AH = reinterpret_cast<const _Float16*>(P0);
      const int lo_off = (R + 1) * ld;
      const int rowi = 16 * rt + i;
      const _Float16* pa[1] = {AH + (rowi < R ? rowi : R) * ld + 8 * q + 32 * k0};
      const Src Wh = make_src(reinterpret_cast<const float*>(planes + gw), (int64_t)d * dff);
      f32x4 acc[1][2] = {{(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}}};
      PipeH3W<1, 2> ph;
      ph.begin(Wh, ch, nks, k0, cnt, cnt > 0, lane);
      ph.run(pa, lo_off, Wh, cnt, acc);
      const int col = 32 * ch + 2 * i;
      for (int sl = 0; sl < ksplit; ++sl) {
        if (ks == sl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + 4 * q + r, rc = row < R ? row : R;
            float2* dst = reinterpret_cast<float2*>(F32 + rc * ldf + col);
            float2 y = make_float2(acc[0][0][r], acc[0][1][r]);
            if (sl > 0) {
              const float2 o = *dst;
              y.x += o.x;
              y.y += o.y;
            }
            *dst = y;
          }
        }
        lds_barrier();
      }
    }
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int c = 4 * lane;
    const bool cok = c < dff;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 b4 = cok ? ld4(bias + c) : z4, w4 = (cok && wdot != nullptr) ? ld4(wdot + c) : z4;
    const Dst df = make_dst_opt(sv, out_off, n0 * dff, (int64_t)vr * dff);
    float4 v[RT];
    float am[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      const float os = OS[r];
      v[q] = cok ? ld4(F32 + rc * ldf + c) : z4;
      v[q] = make_float4(fmaxf(v[q].x * os + b4.x, 0.f), fmaxf(v[q].y * os + b4.y, 0.f), fmaxf(v[q].z * os + b4.z, 0.f), fmaxf(v[q].w * os + b4.w, 0.f));
      buf_st4(df, cok ? (unsigned)c * 4u : ULTR_OOB, (unsigned)(r * dff) * 4u, v[q]);
      am[q] = wdot != nullptr ? (v[q].x * w4.x + v[q].y * w4.y) + (v[q].z * w4.z + v[q].w * w4.w)
                              : fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w));
    }
    if (wdot != nullptr) {
      wave_sum_n<RT>(am);
      const Dst dsc = make_dst(scores + n0, vr);
#pragma unroll
      for (int q = 0; q < RT; ++q) buf_st1(dsc, lane == 0 ? 0u : ULTR_OOB, (unsigned)(wave + NW * q) * 4u, am[q] + bdot);
      return;
    }
    wave_max_n<RT>(am);
    lds_barrier();  // every wave holds its rows: the planes may overwrite them
    _Float16* FH = reinterpret_cast<_Float16*>(P2);
    _Float16* FL = FH + (R + 1) * ldf;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      float rs, inv;
      fb_h3_scale(am[q], rs, inv);
      if (cok) {
        fbh4 hi, lo;
        fb_h3_split4(v[q], rs, hi, lo);
        *reinterpret_cast<fbh4*>(FH + rc * ldf + c) = hi;
        *reinterpret_cast<fbh4*>(FL + rc * ldf + c) = lo;
      }
      if (lane == 0) OS[64 + r] = inv * (1.0f / ULTR_H3_WSCALE);
    }
  };

  SR_BLOCK_STAMP(21);
  product_d(P0, ld, d >> 5, a.gd, d, pbd, OS, false, a.s1);   // s1 = x + (A Wd^T + bd)
  SR_BLOCK_STAMP(22);
  lds_barrier();
  SR_BLOCK_STAMP(23);
  layer_norm(pg1, pb1, a.m1, a.r1, a.out1, true, a.skip_out1 == 0);  // out1 = LN1(s1)
  SR_BLOCK_STAMP(24);
  lds_barrier();
  SR_BLOCK_STAMP(25);
  product_f(a.gf1, pbf1, a.f, nullptr, 0.f);                      // f = relu(out1 Wf1^T + bf1)
  SR_BLOCK_STAMP(26);
  lds_barrier();
  SR_BLOCK_STAMP(27);
  product_d(P2, ldf, dff >> 5, a.gf2, dff, pbf2, OS + 64, true, a.s2);  // s2 = out1 + (f Wf2^T + bf2)
  SR_BLOCK_STAMP(28);
  lds_barrier();
  SR_BLOCK_STAMP(29);
  layer_norm(pg2, pb2, a.m2, a.r2, a.xn, a.head != 0);                    // x' = LN2(s2)
  SR_BLOCK_STAMP(30);
  if (a.head) {
    lds_barrier();
    const float* pbo1 = PV + 6 * d + dff;
    product_f(a.go1, pbo1, a.oh, pbo1 + dff, pbo1[2 * dff]);               // oh = relu(x' Wo1^T + bo1), score = oh . wo2 + bo2
  }
}

// ---------------------------------------------------------------------------------------------------------
// The input side in one launch (round 5): gather + LayerNorm + embedding FFN (SetRank.py:134-135, 146)
// ---------------------------------------------------------------------------------------------------------
//   xg = features[ids],  xn0 = LN_in(xg),  h0 = relu(xn0 W1^T + b1),  x_0 = h0 W2^T + b2      (was: a gather + LayerNorm launch and two GEMMs)
// Same geometry as sr_block_fwd_kernel: a workgroup owns R token rows, the two products run on the fragment-major split-half copies.
struct SrEmbedArgs {
  int R, F, d, dff;
  int64_t T, n_docs;
  int B, L;
  int64_t g_in, b_in, b1, b2;              // float offsets into the parameter vector
  int64_t gw1, gw2;                        // HALF offsets of the fragment copies of W1 [dff][F] and W2 [d][dff]
  int64_t xg, mean_in, rstd_in, xn0, h0, x0;  // float offsets into `saved`; all but x0 < 0: not stored (the scoring forward)
  int p0, p2, pv;                          // float offsets into dynamic LDS
};

__global__ __launch_bounds__(NW * 64) void sr_embed_fwd_kernel(SrEmbedArgs a, const float* __restrict__ params, const float* __restrict__ feats,
                                                              const int32_t* __restrict__ docids, const _Float16* __restrict__ planes,
                                                              float* __restrict__ sv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NT = NW * 64, RT = 4;
  const int R = a.R, F = a.F, d = a.d, dff = a.dff;
  const int K16 = round_up(F, 32), ld0 = K16 + 8, ldf = dff + 8;
  float* P0 = smem + a.p0;   // planes of xn0
  float* P2 = smem + a.p2;   // fp32 partial tiles of h0, then its planes
  float* PV = smem + a.pv;   // g_in | b_in | b1 | b2
  float* OS = PV + 2 * F + dff + d;
  const int tid = threadIdx.x, lane_id = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n0 = (int64_t)blockIdx.x * R;
  const int vr = (int)((a.T - n0) < R ? (a.T - n0) : R);
  const float* pg = PV, *pb = PV + F, *pb1 = PV + 2 * F, *pb2 = PV + 2 * F + dff;

  // ---- gather + LayerNorm: a wave owns rows wave + NW q; lane q < 4 resolves the id of row q ------------------------------------
  {
    const int lane = lane_id;
    for (int e = tid; e < 2 * F + dff + d; e += NT)
      PV[e] = params[e < F ? a.g_in + e : e < 2 * F ? a.b_in + (e - F) : e < 2 * F + dff ? a.b1 + (e - 2 * F) : a.b2 + (e - 2 * F - dff)];
    const int rme = wave + NW * (lane < RT ? lane : 0);
    const bool idok = lane < RT && rme < vr;
    const uint32_t nme = idok ? (uint32_t)(n0 + rme) : 0u;
    const int bb = (int)(nme / (uint32_t)a.L), ll = (int)(nme % (uint32_t)a.L);
    const int id_raw = docids[(int64_t)ll * a.B + bb];
    const int myid = (idok && id_raw >= 0 && id_raw < a.n_docs) ? id_raw : -1;  // PAD -> zero row
    const Src fs = make_src(feats, a.n_docs * F);
    const int c = 4 * lane;
    const bool cok = c < F;
    float4 v[RT];
    float s[RT], qv[RT];
    const Dst dxg = make_dst_opt(sv, a.xg, n0 * F, (int64_t)vr * F);
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int id = __builtin_amdgcn_readlane(myid, q);
      v[q] = buf_ld4(fs, (id >= 0 && cok) ? (unsigned)(((int64_t)id * F + c) * 4) : ULTR_OOB);
    }
    lds_barrier();  // the parameter vectors are in LDS
    const float invF = 1.0f / (float)F;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      buf_st4(dxg, cok ? (unsigned)c * 4u : ULTR_OOB, (unsigned)((wave + NW * q) * F) * 4u, v[q]);
      s[q] = (v[q].x + v[q].y) + (v[q].z + v[q].w);
    }
    wave_sum_n<RT>(s);
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      s[q] *= invF;
      if (cok) {
        v[q].x -= s[q]; v[q].y -= s[q]; v[q].z -= s[q]; v[q].w -= s[q];
      }
      qv[q] = (v[q].x * v[q].x + v[q].y * v[q].y) + (v[q].z * v[q].z + v[q].w * v[q].w);
    }
    wave_sum_n<RT>(qv);
    const Dst dmean = make_dst_opt(sv, a.mean_in, n0, vr), drstd = make_dst_opt(sv, a.rstd_in, n0, vr);
    const Dst dxn = make_dst_opt(sv, a.xn0, n0 * F, (int64_t)vr * F);
    const unsigned l0 = lane == 0 ? 0u : ULTR_OOB;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g4 = cok ? ld4(pg + c) : z4, b4 = cok ? ld4(pb + c) : z4;
    float am[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q;
      const float rstd = 1.0f / sqrtf(qv[q] * invF + SR_EPS);
      v[q] = make_float4(v[q].x * rstd * g4.x + b4.x, v[q].y * rstd * g4.y + b4.y, v[q].z * rstd * g4.z + b4.z, v[q].w * rstd * g4.w + b4.w);
      buf_st4(dxn, cok ? (unsigned)c * 4u : ULTR_OOB, (unsigned)(r * F) * 4u, v[q]);
      buf_st1(dmean, l0, (unsigned)r * 4u, s[q]);
      buf_st1(drstd, l0, (unsigned)r * 4u, rstd);
      am[q] = fmaxf(fmaxf(fabsf(v[q].x), fabsf(v[q].y)), fmaxf(fabsf(v[q].z), fabsf(v[q].w)));
    }
    wave_max_n<RT>(am);
    _Float16* AH = reinterpret_cast<_Float16*>(P0);
    _Float16* AL = AH + (R + 1) * ld0;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      float rs, inv;
      fb_h3_scale(am[q], rs, inv);
      if (c < K16) {  // (columns F .. K16 - 1: zeros - v is 0 * rstd * 0 + 0 there)
        fbh4 hi, lo;
        fb_h3_split4(v[q], rs, hi, lo);
        *reinterpret_cast<fbh4*>(AH + rc * ld0 + c) = hi;
        *reinterpret_cast<fbh4*>(AL + rc * ld0 + c) = lo;
      }
      if (lane == 0) OS[r] = inv * (1.0f / ULTR_H3_WSCALE);
    }
  }
  lds_barrier();
  // ---- h0 = relu(xn0 W1^T + b1): wave = (row tile, chunk, slice of the contraction) -> fp32 partial tiles in P2; then the owner waves
  {
    float* F32 = P2;
    {
      int lane = lane_id;
      asm volatile("" : "+v"(lane));
      const int i = lane & 15, q = lane >> 4, nks = K16 >> 5, nchf = dff >> 5, ksplit = 4 / nchf;
      const int rt = wave >> 2;
      int ch = wave & 3, ks = 0;
      while (ch >= nchf) { ch -= nchf; ++ks; }
      const int len = (nks + ksplit - 1) / ksplit, k0 = ks * len;
      const int cnt = k0 >= nks ? 0 : (k0 + len < nks ? len : nks - k0);
      const _Float16* AH = reinterpret_cast<const _Float16*>(P0);
      const int lo_off = (R + 1) * ld0;
      const int rowi = 16 * rt + i;
      const _Float16* pa[1] = {AH + (rowi < R ? rowi : R) * ld0 + 8 * q + 32 * k0};
      const Src Wh = make_src(reinterpret_cast<const float*>(planes + a.gw1), (int64_t)K16 * dff);
      f32x4 acc[1][2] = {{(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}}};
      PipeH3W<1, 2> ph;
      ph.begin(Wh, ch, nks, k0, cnt, cnt > 0, lane);
      ph.run(pa, lo_off, Wh, cnt, acc);
      const int col = 32 * ch + 2 * i;
      for (int sl = 0; sl < ksplit; ++sl) {
        if (ks == sl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + 4 * q + r, rc = row < R ? row : R;
            float2* dst = reinterpret_cast<float2*>(F32 + rc * ldf + col);
            float2 y = make_float2(acc[0][0][r], acc[0][1][r]);
            if (sl > 0) {
              const float2 o = *dst;
              y.x += o.x;
              y.y += o.y;
            }
            *dst = y;
          }
        }
        lds_barrier();
      }
    }
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int c = 4 * lane;
    const bool cok = c < dff;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 b4 = cok ? ld4(pb1 + c) : z4;
    const Dst dh = make_dst_opt(sv, a.h0, n0 * dff, (int64_t)vr * dff);
    float4 v[RT];
    float am[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      const float os = OS[r];
      v[q] = cok ? ld4(F32 + rc * ldf + c) : z4;
      v[q] = make_float4(fmaxf(v[q].x * os + b4.x, 0.f), fmaxf(v[q].y * os + b4.y, 0.f), fmaxf(v[q].z * os + b4.z, 0.f), fmaxf(v[q].w * os + b4.w, 0.f));
      buf_st4(dh, cok ? (unsigned)c * 4u : ULTR_OOB, (unsigned)(r * dff) * 4u, v[q]);
      am[q] = fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w));
    }
    wave_max_n<RT>(am);
    lds_barrier();  // every wave holds its rows: the planes may overwrite them
    _Float16* FH = reinterpret_cast<_Float16*>(P2);
    _Float16* FL = FH + (R + 1) * ldf;
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      const int r = wave + NW * q, rc = r < R ? r : R;
      float rs, inv;
      fb_h3_scale(am[q], rs, inv);
      if (cok) {
        fbh4 hi, lo;
        fb_h3_split4(v[q], rs, hi, lo);
        *reinterpret_cast<fbh4*>(FH + rc * ldf + c) = hi;
        *reinterpret_cast<fbh4*>(FL + rc * ldf + c) = lo;
      }
      if (lane == 0) OS[64 + r] = inv * (1.0f / ULTR_H3_WSCALE);
    }
  }
  lds_barrier();
  // ---- x_0 = h0 W2^T + b2: wave = (32-column chunk, pair of row tiles), straight to `saved` --------------------------------------
  {
    int lane = lane_id;
    asm volatile("" : "+v"(lane));
    const int nch = d >> 5, nks = dff >> 5;
    const int ch = wave & 7, g = wave >> 3;
    const bool has = ch < nch;
    const int i = lane & 15, q = lane >> 4;
    const _Float16* AH = reinterpret_cast<const _Float16*>(P2);
    const int lo_off = (R + 1) * ldf;
    const _Float16* pa[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 16 * (2 * g + t) + i;
      pa[t] = AH + (row < R ? row : R) * ldf + 8 * q;
    }
    const Src Wh = make_src(reinterpret_cast<const float*>(planes + a.gw2), (int64_t)dff * d);
    PipeH3W<2, 2> ph;
    ph.begin(Wh, ch, nks, 0, nks, has, lane);
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) acc[t][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ph.run(pa, lo_off, Wh, has ? nks : 0, acc);
    if (has) {
      const int col = 32 * ch + 2 * i;
      const Dst dout = make_dst(sv + a.x0 + n0 * d, (int64_t)vr * d);
      const float2 bv = *reinterpret_cast<const float2*>(pb2 + col);
      const unsigned gv = (unsigned)(4 * q * d + 2 * i) * 4u;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 o4 = ld4(OS + 64 + 16 * (2 * g + t) + 4 * q);
        const float o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          buf_st2(dout, gv, (unsigned)((16 * (2 * g + t) + r) * d + 32 * ch) * 4u,
                  make_float2(acc[t][0][r] * o[r] + bv.x, acc[t][1][r] * o[r] + bv.y));
      }
    }
  }
}


// the fields sr_block_fwd_kernel and sr_fwd_block_kernel share (SrBlockArgs / SrFwdBlockArgs): block l's offsets into the parameter vector,
// the planes and `saved`, and the output FFN's where it rides with the last block.  On a route with a block kernel every fragment-major
// copy asked for here exists (sr_make_plan built them for these widths; the planes are on).
template <typename Args>
void fill_block_args(Args& a, const SrCall& c, const SrRoute& rt, int l) {
  const SrPlan& p = c.p;
  const int d = p.d, dff = p.dff;
  const SrLayer& y = p.lay[l];
  memset(&a, 0, sizeof(a));
  a.d = d; a.dff = dff; a.T = p.T;
  a.bd = y.bd; a.bf1 = y.bf1; a.bf2 = y.bf2; a.g1 = y.g1; a.b1 = y.b1; a.g2 = y.g2; a.b2 = y.b2;
  a.gd = c.split(y.wd, d, d)->g_off; a.gf1 = c.split(y.wf1, dff, d)->g_off; a.gf2 = c.split(y.wf2, d, dff)->g_off;
  a.A = p.sv_A[l]; a.x = p.sv_x[l]; a.s1 = p.sv_s1[l]; a.m1 = p.sv_m1[l]; a.r1 = p.sv_r1[l]; a.out1 = p.sv_out1[l]; a.f = p.sv_f[l];
  a.s2 = p.sv_s2[l]; a.m2 = p.sv_m2[l]; a.r2 = p.sv_r2[l]; a.xn = p.sv_x[l + 1];
  a.skip_out1 = rt.skip_out1;
  if (rt.head_rides && l == p.nl - 1) {
    a.head = 1;
    a.go1 = c.split(p.wo1, dff, d)->g_off; a.bo1 = p.bo1; a.wo2 = p.wo2; a.bo2 = p.bo2; a.oh = p.sv_oh;
  }
  if (p.score) a.s1 = a.out1 = a.f = a.s2 = a.oh = -1;  // no backward follows: the rows stay in LDS (the plan's buffers for them serve the separate launches)
}

}  // namespace

// everything of encoder block l behind the attention as the ONE launch the route names (rt.block: _ROUND5 or _PERSISTENT); on the last
// block with rt.head_rides the output FFN and the scores as well
int sr_block_fwd(const SrCall& c, const SrRoute& rt, int l, float* scores) {
  const SrPlan& p = c.p;
  if (rt.block == SR_BLOCK_PERSISTENT) {  // ONE persistent 8-wave workgroup per CU over tiles of rt.R rows (sr_fwd_block_kernel, ultr_sr_fwd.hip)
    SrFwdBlockArgs fa;
    fill_block_args(fa, c, rt, l);
    fa.R = rt.R; fa.ntiles = rt.tiles;
    return sr_fwd_block_launch(fa, rt.nwg, c.params, c.planes, c.sv, scores, c.st);
  }
  const int d = p.d, dff = p.dff, R = rt.block_R;
  SrBlockArgs a;
  fill_block_args(a, c, rt, l);
  a.R = R;
  a.p0 = 0;
  a.p1 = (R + 1) * (d + 8);
  a.p2 = 2 * a.p1;
  a.pv = a.p2 + (R + 1) * (dff + 8);
#ifdef ULTR_TRACE
  a.trace = sr_gemm_trace_slots();
#endif
  const size_t lds = (size_t)(a.pv + 6 * d + 3 * dff + 4 + 128) * sizeof(float);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(sr_block_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  hipLaunchKernelGGL(sr_block_fwd_kernel, dim3((unsigned)((p.T + R - 1) / R)), dim3(NW * 64), lds, c.st, a, c.params, c.planes, c.sv, scores);
  return (int)hipGetLastError();
}

// gather + input LayerNorm + embedding FFN as one launch (rt.embed; the caller has checked the features pointer)
int sr_embed_fwd(const SrCall& c, const SrRoute& rt, const float* feats, const int32_t* docids, int64_t n_docs, int batch, int L) {
  const SrPlan& p = c.p;
  const int F = p.F, d = p.d, dff = p.dff, R = rt.embed_R;
  const int K16 = (F + 31) / 32 * 32;
  SrEmbedArgs a;
  memset(&a, 0, sizeof(a));
  a.R = R; a.F = F; a.d = d; a.dff = dff; a.T = p.T; a.n_docs = n_docs; a.B = batch; a.L = L;
  a.g_in = p.g_in; a.b_in = p.b_in; a.b1 = p.b1; a.b2 = p.b2;
  a.gw1 = c.split(p.w1, dff, F)->g_off; a.gw2 = c.split(p.w2, d, dff)->g_off;
  a.xg = p.sv_xg; a.mean_in = p.sv_mean_in; a.rstd_in = p.sv_rstd_in; a.xn0 = p.sv_xn0; a.h0 = p.sv_h0; a.x0 = p.sv_x[0];
  if (p.score) a.xn0 = a.h0 = -1;  // (xg and the statistics: -1 in the scoring plan itself)
  a.p0 = 0;
  a.p2 = (R + 1) * (K16 + 8);
  a.pv = a.p2 + (R + 1) * (dff + 8);
  const size_t lds = (size_t)(a.pv + 2 * F + dff + d + 128) * sizeof(float);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(sr_embed_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  hipLaunchKernelGGL(sr_embed_fwd_kernel, dim3((unsigned)((p.T + R - 1) / R)), dim3(NW * 64), lds, c.st, a, c.params, feats, docids, c.planes, c.sv);
  return (int)hipGetLastError();
}
