// ultr_sr_attn_long.hip - SetRank's self-attention for lists the one-pass kernels of ultr_sr_attn.hip do not take: the FORWARD beyond 256
// documents (ULTR_SR_ATTN_LONG_MIN lowers the hand-over point for tests and measurement) and, for a model that asks for it
// (ULTR_MODEL_SR_STREAM_BWD), the BACKWARD beyond the one-pass backward's 128 / 120.  The reference has no list bound
// (ranking_model/SetRank.py:156-191, 243-251: unmasked attention over however many documents the list has); validation, test and
// reranking score max_candidate_num positions, 1251 at MSLR-WEB30K, and DirectLabelFeed trains at them.
//
// The keys STREAM: a workgroup owns a block of queries of one (list, head) and walks the list in key tiles staged into LDS; per query
// it keeps a running maximum m and sum s of exp(score - m) and the unnormalised P.V accumulator, all rescaled by exp(m_old - m_new) when
// a tile raises the maximum; the division by s happens once, at the end.  Nothing in LDS or registers grows with the list size.
// Error model: with the final maximum M every probability is exp(S - m_k) prod_j exp(m_j - m_{j+1}) instead of exp(S - M) - one
// rounding per tile in which the maximum ROSE (a factor of exactly 1 otherwise), so at most log-many in practice and never more than
// the tile count; the sums add tile partials in key order.  The order is a pure function of (L, DH): no atomics, the same bits
// run to run.  A and lse keep the layouts of the one-pass kernels, so `saved` stays a complete record.
// The backward (second half of this file) streams PARTNER tiles: the forward left lse, so there is no running maximum and no rescale there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_sr_attn.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// fp32 matrix cores: head depth 16 / 32 / 64, 16-byte aligned head slices
// ---------------------------------------------------------------------------------------------------------
// One workgroup = 8 waves x 16 queries of one (list, head); key tiles of 128 rows in sr_stage_head's layout ([rows][DH + 4] floats,
// zero rows past L), double-buffered: the next tile's rows are requested into registers before the current tile's products and
// written to the other buffer behind them - one barrier per tile.  A tile is the K operand of the scores and the V operand of P.V
// (q = k = v).  Per tile and wave, exactly the one-pass kernel's register tiling: the TRANSPOSED score tiles D[key][query] (sr_tile_nt),
// so lane (i, q) holds the scores of ITS query i for keys {16 t + 4 q + r} - the row statistics live in the 4 lanes {i, i + 16, i + 32,
// i + 48} - and the probabilities are already the A operand of P.V.  The accumulator o[c] is D[query 4 q + r][column 16 c + i]: its
// rescale factor belongs to another lane's query and is fetched across lanes (4 moves per tile of 128 keys).
// LDS: 2 x 128 x (DH + 4) floats = 20 / 36 / 68 KiB - two workgroups per CU at head depth 64, which the registers must allow too
// (four waves per SIMD: at most 128, amdgpu_waves_per_eu below; without it head depth 64 took 144).
constexpr int SRL_NW = 8, SRL_NTHR = SRL_NW * 64, SRL_QB = 16 * SRL_NW, SRL_TK = 128, SRL_NT = SRL_TK / 16;

template <int DH>
__global__ __launch_bounds__(SRL_NTHR) __attribute__((amdgpu_waves_per_eu(4, 8))) void sr_attn_fwd_long_kernel(
    const float* __restrict__ x, int batch, int L, int d, int nqb, float* __restrict__ A, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KQ = DH / 4, LDX = DH + 4, NC = DH / 16, NF = DH / 16, RT = DH / 4;
  constexpr int NST = SRL_TK * RT / SRL_NTHR;  // float4s of a key tile per thread (DH / 16)
  static_assert(NST * SRL_NTHR == SRL_TK * RT, "a tile is a whole number of float4s per thread");
  // grid.x = query blocks x a chunk of lists, grid.z = list chunks (SrlGrid); the last chunk may be ragged: whole workgroups leave
  const int qb = blockIdx.x % nqb, b = blockIdx.z * (gridDim.x / nqb) + blockIdx.x / nqb, h = blockIdx.y, H = gridDim.y;
  if (b >= batch) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int64_t base = (int64_t)b * L * d + h * DH;
  const int q0 = qb * SRL_QB + wave * 16;  // this wave's query block
  const bool live = q0 < L;                // (a wave without queries still stages tiles and meets the barriers)
  float4 st[NST];
  auto tile_load = [&](int k0) {  // rows k0 .. k0 + 127 of the head slice, zero past L
#pragma unroll
    for (int k = 0; k < NST; ++k) {
      const int e = tid + SRL_NTHR * k, r = e / RT, c4 = (e - r * RT) * 4;
      st[k] = (k0 + r < L) ? ld4(x + base + (int64_t)(k0 + r) * d + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto tile_store = [&](float* xs) {
#pragma unroll
    for (int k = 0; k < NST; ++k) {
      const int e = tid + SRL_NTHR * k, r = e / RT, c4 = (e - r * RT) * 4;
      st4(xs + r * LDX + c4, st[k]);
    }
  };
  tile_load(0);
  tile_store(smem);
  float4 bq[NF];  // this wave's query block, straight from global memory: lane (i, q) holds x[q0 + i][q KQ + 4 f ..]; zero past L
#pragma unroll
  for (int f = 0; f < NF; ++f)
    bq[f] = (q0 + i < L) ? ld4(x + base + (int64_t)(q0 + i) * d + q * KQ + 4 * f) : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const float scale = 1.0f / sqrtf((float)DH);
  const float c1 = scale * 1.44269504088896341f;  // exp(scale * (s - m)) = 2^(s * c1 - m * c1), as in the one-pass kernel
  float m = -INFINITY;  // running maximum of the RAW scores of query i (scale > 0); the same in the 4 lanes of the query
  float m2 = 0.f;       // fl(m * c1): the exponent offset the held probabilities are relative to, EXACTLY (set by every tile)
  float sum = 0.f;      // this lane's share of the running sum (its keys 4 q + r of every block); joined over the 4 lanes at the end
  f32x4 o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntile = (L + SRL_TK - 1) / SRL_TK;
  for (int kt = 0; kt < ntile; ++kt) {
    const int k0 = kt * SRL_TK;
    float* xs = smem + (kt & 1) * (SRL_TK * LDX);
    if (kt + 1 < ntile) tile_load(k0 + SRL_TK);
    if (live) {
      const int nb = min(SRL_NT, (L - k0 + 15) / 16);  // 16-key blocks of this tile that hold a key (>= 1)
      f32x4 pr[SRL_NT];  // pr[t][r]: key k0 + 16 t + 4 q + r, query = this lane's i
      float mt = -INFINITY;
#pragma unroll
      for (int t = 0; t < SRL_NT; ++t) {
        if (t < nb) {
          pr[t] = sr_tile_nt<DH>(xs + (t * 16 + i) * LDX + q * KQ, bq);
          // The zero rows past L score 0.  In the one-pass kernel that is never above the query's own |x_i|^2; here the query's own
          // key may sit in another tile and every real score of this one may be negative: masked BEFORE the maximum is taken.
          // (-inf also gives the probability 2^-inf = 0 below: one mask for the maximum and the sum.)
          if (k0 + t * 16 + 16 > L) {
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[t][r] = (k0 + t * 16 + 4 * q + r < L) ? pr[t][r] : -INFINITY;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) mt = fmaxf(mt, pr[t][r]);
        }
      }
      mt = quad_max(mt);  // finite: key k0 is a real key of every tile
      const float mn = fmaxf(m, mt), mn2 = mn * c1;
      // what the previous tiles hold is relative to 2^-m2: rescale by 2^(m2 - mn2) <= 1, formed from the two ROUNDED offsets - exactly 1
      // when the maximum did not rise.  (fma(m, c1, -mn2) would leave the rounding residue of m * c1 there, a factor 2^delta of one sign
      // in every later tile: an error that grows with the tile count.)  The first tile has nothing to rescale and m = -inf; the
      // factor is named 0 there, not computed from infinities.
      const float alpha = (kt == 0) ? 0.f : __builtin_amdgcn_exp2f(m2 - mn2);
      m2 = mn2;
      m = mn;
      float ts = 0.f;
#pragma unroll
      for (int t = 0; t < SRL_NT; ++t) {
        if (t < nb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pr[t][r] = __builtin_amdgcn_exp2f(fmaf(pr[t][r], c1, -mn2));
            ts += pr[t][r];
          }
        }
      }
      sum = fmaf(sum, alpha, ts);
      if (kt > 0) {  // o[c][r] belongs to query 4 q + r, whose factor lane 4 q + r holds
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ar = __shfl(alpha, 4 * q + r);
#pragma unroll
          for (int c = 0; c < NC; ++c) o[c][r] *= ar;
        }
      }
#pragma unroll
      for (int t = 0; t < SRL_NT; ++t) {
        if (t < nb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* vr = xs + (t * 16 + 4 * q + r) * LDX + i;
#pragma unroll
            for (int c = 0; c < NC; ++c) o[c] = mfma16(pr[t][r], vr[c * 16], o[c]);
          }
        }
      }
    }
    // the other buffer was last read in the previous trip, which every wave left through the barrier below
    if (kt + 1 < ntile) tile_store(smem + ((kt + 1) & 1) * (SRL_TK * LDX));
    __syncthreads();
  }
  if (!live) return;
  sum = quad_sum(sum);
  const float inv = 1.0f / sum;
  // row statistic in the one-pass kernel's form: P[i][j] = exp(S[i][j] - lse[i])
  if (lse != nullptr && q == 0 && q0 + i < L) lse[((int64_t)b * L + q0 + i) * H + h] = m * scale + logf(sum);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * q + r);
    const int row = q0 + 4 * q + r;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (row < L) A[base + (int64_t)row * d + c * 16 + i] = o[c][r] * ir;
  }
}

// ---------------------------------------------------------------------------------------------------------
// every other head depth (and ULTR_SR_SCALAR_ATTN=1): the same recurrence, scalar.  Slow; correct at any (L, dh).
// ---------------------------------------------------------------------------------------------------------
// One workgroup = 4 waves x 4 queries of one (list, head); key tiles of 64 rows, one key per lane.  Per query the wave holds m and the
// sum as wave-uniform values; the unnormalised output row lives in LDS (the head depth is not a compile-time constant).
// LDS: (64 + 16) (dh + 1) + 16 dh + 4 x 64 floats - a function of dh alone.
constexpr int SRS_QW = 4, SRS_QB = 4 * SRS_QW, SRS_TK = 64;

size_t srs_lds_bytes(int dh) { return ((size_t)(SRS_TK + SRS_QB) * (dh + 1) + (size_t)SRS_QB * dh + 4 * SRS_TK) * sizeof(float); }

__global__ __launch_bounds__(256) void sr_attn_fwd_long_scalar_kernel(const float* __restrict__ x, int batch, int L, int d, int dh, int nqb,
                                                                      float* __restrict__ A, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = dh + 1;
  float* ks = smem;                   // [64][dh + 1] the key tile, zero rows past L
  float* qs = ks + SRS_TK * ldx;      // [16][dh + 1] the query block
  float* os = qs + SRS_QB * ldx;      // [16][dh]     unnormalised outputs
  float* ps = os + SRS_QB * dh;       // [4 waves][64] probabilities of the wave's current query
  // grid.x = query blocks x a chunk of lists, grid.z = list chunks (SrlGrid); the last chunk may be ragged: whole workgroups leave
  const int qb = blockIdx.x % nqb, b = blockIdx.z * (gridDim.x / nqb) + blockIdx.x / nqb, h = blockIdx.y, H = gridDim.y;
  if (b >= batch) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = qb * SRS_QB;
  const float* xb = x + (int64_t)b * L * d + h * dh;
  for (int e = tid; e < SRS_QB * dh; e += 256) {
    const int r = e / dh, c = e - r * dh;
    qs[r * ldx + c] = (q0 + r < L) ? xb[(int64_t)(q0 + r) * d + c] : 0.f;
    os[e] = 0.f;
  }
  const float scale = 1.0f / sqrtf((float)dh);
  float m[SRS_QW], sum[SRS_QW];  // of the SCALED scores
#pragma unroll
  for (int u = 0; u < SRS_QW; ++u) {
    m[u] = -INFINITY;
    sum[u] = 0.f;
  }
  float* pw = ps + wave * SRS_TK;
  for (int k0 = 0; k0 < L; k0 += SRS_TK) {
    __syncthreads();  // the previous tile's readers are done (first trip: nothing to wait for)
    for (int e = tid; e < SRS_TK * dh; e += 256) {
      const int r = e / dh, c = e - r * dh;
      ks[r * ldx + c] = (k0 + r < L) ? xb[(int64_t)(k0 + r) * d + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SRS_QW; ++u) {
      const int qi = wave * SRS_QW + u;
      if (q0 + qi < L) {  // wave-uniform
        float acc = 0.f;
        for (int c = 0; c < dh; ++c) acc += qs[qi * ldx + c] * ks[lane * ldx + c];
        const float sc = (k0 + lane < L) ? acc * scale : -INFINITY;  // masked before the maximum (see the matrix-core kernel)
        const float mn = fmaxf(m[u], wave_max(sc));                  // finite: key k0 is real
        const float alpha = (k0 == 0) ? 0.f : expf(m[u] - mn);       // first tile: nothing to rescale, m = -inf
        const float p = expf(sc - mn);                               // 0 for a masked key
        sum[u] = sum[u] * alpha + wave_sum(p);
        m[u] = mn;
        pw[lane] = p;
        __builtin_amdgcn_wave_barrier();
        for (int c = lane; c < dh; c += 64) {
          float a = os[qi * dh + c] * alpha;
          for (int j = 0; j < SRS_TK; ++j) a += pw[j] * ks[j * ldx + c];
          os[qi * dh + c] = a;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
#pragma unroll
  for (int u = 0; u < SRS_QW; ++u) {
    const int row = q0 + wave * SRS_QW + u;
    if (row < L) {  // the wave reads the output rows it wrote itself
      for (int c = lane; c < dh; c += 64) A[((int64_t)b * L + row) * d + h * dh + c] = os[(wave * SRS_QW + u) * dh + c] / sum[u];
      if (lse != nullptr && lane == 0) lse[((int64_t)b * L + row) * H + h] = m[u] + logf(sum[u]);
    }
  }
}

// grid = (query blocks x lists, heads, list chunks): a list's query blocks are neighbours, they read the same keys.  HIP bounds
// gridDim.x * blockDim.x at 2^32, so x takes as many whole lists as fit under it and z the chunks of lists; ULTR_E_UNSUPPORTED only where
// ONE list has more query blocks than that (2^29 documents and more) or the chunks exceed gridDim.z - both beyond T <= 0x7fffffff / 4.
struct SrlGrid {
  int nqb;
  dim3 grid;
};
int srl_grid(int batch, int L, int H, int queries_per_wg, int threads, SrlGrid* g) {
  const int64_t max_x = 0xffffffffLL / threads;
  const int64_t nqb = ((int64_t)L + queries_per_wg - 1) / queries_per_wg;
  if (nqb > max_x) return ULTR_E_UNSUPPORTED;
  const int64_t lists = max_x / nqb < batch ? max_x / nqb : batch;
  const int64_t nz = (batch + lists - 1) / lists;
  if (nz > 65535) return ULTR_E_UNSUPPORTED;
  g->nqb = (int)nqb;
  g->grid = dim3((unsigned)(nqb * lists), (unsigned)H, (unsigned)nz);
  return 0;
}

template <int DH>
int srl_launch_mfma(const SrAttnShape& p, const float* x, int batch, int L, float* A, float* lse, hipStream_t st) {
  SrlGrid g;
  int rc = srl_grid(batch, L, p.H, SRL_QB, SRL_NTHR, &g);
  if (rc != 0) return rc;
  const size_t lds = (size_t)2 * SRL_TK * (DH + 4) * sizeof(float);
  rc = set_dyn_lds(sr_attn_fwd_long_kernel<DH>, lds);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(sr_attn_fwd_long_kernel<DH>, g.grid, dim3(SRL_NTHR), lds, st, x, batch, L, p.d, g.nqb, A, lse);
  return 0;
}


// ---------------------------------------------------------------------------------------------------------
// BACKWARD.  dx_h += scale (dS x + dS^T x) + P^T dA  with  P_ij = exp(scale S_ij - lse_i),  dP_ij = dA_i . x_j,  t_i = dA_i . A_i,
// dS_ij = P_ij (dP_ij - t_i)   (q = k = v = x_h, S symmetric; ultr_sr_attn.hip: sr_attn_bwd_mfma_kernel).
// ---------------------------------------------------------------------------------------------------------
// lse comes from the forward: no running maximum, no rescale, P <= 1 up to rounding.  t[T, H] comes from a pre-pass over dA and A (one
// read of each; staging it per tile would read A once per token block) into the caller's workspace.
// DH > 0: the RT = DH / 4 threads of a (token, head) are consecutive lanes and join by butterfly - the one-pass kernel's order of the
// same sum.  DH = 0: one thread per (token, head), any head depth.
template <int DH>
__global__ __launch_bounds__(256) void sr_attn_t_kernel(const float* __restrict__ dA, const float* __restrict__ Aout, int64_t T, int d, int dh, int H,
                                                         float* __restrict__ t) {
  if (DH > 0) {
    constexpr int RT = DH > 0 ? DH / 4 : 1;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (whole groups of RT lanes: 256 and the grid's total are multiples of RT)
    const int64_t g = e / RT;                                   // (token, head)
    const int c4 = (int)(e - g * RT) * 4;
    const int64_t row = g / H;
    const int h = (int)(g - row * H);
    const bool ok = row < T;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 gv = ok ? ld4(dA + row * d + h * DH + c4) : z4;
    const float4 av = ok ? ld4(Aout + row * d + h * DH + c4) : z4;
    float tt = gv.x * av.x + gv.y * av.y + gv.z * av.z + gv.w * av.w;
#pragma unroll
    for (int m = 1; m < RT; m <<= 1) tt += __shfl_xor(tt, m);
    if (ok && c4 == 0) t[g] = tt;
  } else {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= T * H) return;
    const int64_t row = g / H;
    const int h = (int)(g - row * H);
    const float* gp = dA + row * d + h * dh;
    const float* ap = Aout + row * d + h * dh;
    float tt = 0.f;
    for (int c = 0; c < dh; ++c) tt += gp[c] * ap[c];
    t[g] = tt;
  }
}

// fp32 matrix cores: the one-pass sr_attn_bwd_mfma_kernel with the partner blocks streamed.  One workgroup = 8 waves x 16 tokens of one
// (list, head); a wave owns its 16 tokens in BOTH roles - its x / dA fragments, lse and t stay in registers - and meets every token of
// the list as partner: tiles of 128 rows of x and dA in sr_stage_head's layout ([rows][DH + 4], zero rows past L) with their
// lse * log2(e) (+inf past L: P = 0) and t.  Per partner block of 16 the one-pass kernel's six products: the transposed score tile
// (both roles), dP^T and dP, then dq + dk and dv in separate chains summed at the end.  Padding QUERIES have lse = +inf; padding KEYS
// exist only in the last block of the last tile and are masked there; blocks of the last tile without a token are not walked.
// Tiles are double-buffered as in the forward: the next tile is requested into registers before the current products and written to
// the other LDS buffer behind them, one barrier per tile.  LDS: 2 x (2 x 128 x (DH + 4) + 256) floats = 42 / 74 / 138 KiB.
// Both buffers in LDS, not one in LDS and one held in registers across a second barrier: the registers bound the occupancy before the
// LDS does.  Head depth 16 / 32 take 86 / 127 registers (four waves per SIMD, two workgroups per CU, 84 / 148 KiB of LDS between them);
// head depth 64 takes 205 with a tile in flight (held to 128 it spilled 117 of them), so it runs two waves per SIMD - one workgroup
// per CU, which the 138 KiB allow - rather than spill.
// A workgroup writes its own 128 rows of dx and nothing else: no atomics, the order of every sum a pure function of (L, DH).
template <int DH>
__global__ __launch_bounds__(SRL_NTHR) __attribute__((amdgpu_waves_per_eu(DH == 64 ? 2 : 4, 8))) void sr_attn_bwd_long_kernel(
    const float* __restrict__ x, const float* __restrict__ dA, const float* __restrict__ lse, const float* __restrict__ tws, int batch, int L,
    int d, int nqb, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KQ = DH / 4, LDX = DH + 4, NC = DH / 16, NF = DH / 16, RT = DH / 4;
  constexpr int NST = SRL_TK * RT / SRL_NTHR;           // float4s of one tile plane per thread (DH / 16)
  constexpr int BUF = 2 * SRL_TK * LDX + 2 * SRL_TK;    // floats of one buffer: x | dA | lse * log2(e) | t
  static_assert(NST * SRL_NTHR == SRL_TK * RT, "a tile is a whole number of float4s per thread");
  const int qb = blockIdx.x % nqb, b = blockIdx.z * (gridDim.x / nqb) + blockIdx.x / nqb, h = blockIdx.y, H = gridDim.y;
  if (b >= batch) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int64_t base = (int64_t)b * L * d + h * DH;
  const int64_t sbase = (int64_t)b * L;  // row of the [T, H] statistics
  const int q0 = qb * SRL_QB + wave * 16;  // this wave's own block
  const bool live = q0 < L;                // (a wave without tokens still stages tiles and meets the barriers)
  constexpr float LOG2E = 1.44269504088896341f;
  float4 sx[NST], sg[NST];
  auto tile_load = [&](int k0) {  // requests rows k0 .. k0 + 127 of the head slices, zero past L
    // (the tile's origin is wave-uniform, 64-bit; what a thread adds stays below 129 d: 32 bits, one register per request instead of
    // a pointer pair per plane held across the products)
    const float* xt = x + base + (int64_t)k0 * d;
    const float* gt = dA + base + (int64_t)k0 * d;
#pragma unroll
    for (int k = 0; k < NST; ++k) {
      const int e = tid + SRL_NTHR * k, r = e / RT, c4 = (e - r * RT) * 4;
      const bool ok = k0 + r < L;
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const unsigned off = (unsigned)(r * d + c4);
      sx[k] = ok ? ld4(xt + off) : z4;
      sg[k] = ok ? ld4(gt + off) : z4;
    }
  };
  // ... and stores them behind the products; the first two waves fetch the tile's 128 row statistics here, not before the products:
  // two more registers held across them made head depth 32 spill at four waves per SIMD
  auto tile_store = [&](float* buf, int k0) {
#pragma unroll
    for (int k = 0; k < NST; ++k) {
      const int e = tid + SRL_NTHR * k, r = e / RT, c4 = (e - r * RT) * 4;
      st4(buf + r * LDX + c4, sx[k]);
      st4(buf + SRL_TK * LDX + r * LDX + c4, sg[k]);
    }
    if (tid < SRL_TK) {
      const bool ok = k0 + tid < L;
      buf[2 * SRL_TK * LDX + tid] = ok ? lse[(sbase + k0 + tid) * H + h] * LOG2E : INFINITY;
      buf[2 * SRL_TK * LDX + SRL_TK + tid] = ok ? tws[(sbase + k0 + tid) * H + h] : 0.f;
    }
  };
  tile_load(0);
  tile_store(smem, 0);
  float4 bx[NF], bg[NF];  // this wave's block, straight from global memory: lane (i, q) holds x / dA [q0 + i][q KQ + 4 f ..]; zero past L
  const bool own_ok = q0 + i < L;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    bx[f] = own_ok ? ld4(x + base + (int64_t)(q0 + i) * d + q * KQ + 4 * f) : z4;
    bg[f] = own_ok ? ld4(dA + base + (int64_t)(q0 + i) * d + q * KQ + 4 * f) : z4;
  }
  const float l_own = own_ok ? lse[(sbase + q0 + i) * H + h] * LOG2E : INFINITY;
  const float t_own = own_ok ? tws[(sbase + q0 + i) * H + h] : 0.f;
  __syncthreads();
  const float scale = 1.0f / sqrtf((float)DH);
  const float c1 = scale * LOG2E;  // P = 2^(S * scale * log2(e) - lse * log2(e)): one fma + v_exp_f32, as in the one-pass kernel
  f32x4 acc[NC], acv[NC];          // dq + dk, dv: separate chains, summed at the end
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = acv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntile = (L + SRL_TK - 1) / SRL_TK;
  for (int kt = 0; kt < ntile; ++kt) {
    const int k0 = kt * SRL_TK;
    const float* xs = smem + (kt & 1) * BUF;
    const float* das = xs + SRL_TK * LDX;
    const float* st_l = das + SRL_TK * LDX;
    const float* st_t = st_l + SRL_TK;
    if (kt + 1 < ntile) tile_load(k0 + SRL_TK);
    if (live) {
      auto partner_block = [&](int t, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const float* xrow = xs + (t * 16 + i) * LDX + q * KQ;
        const float* grow = das + (t * 16 + i) * LDX + q * KQ;
        //   sc  = S[partner 16 t + 4 q + r][own i]  (symmetric: serves both roles)
        //   dpt = dP^T[key partner][query own i] = x[key] . dA[query]
        //   dpn = dP[query partner][key own i]   = dA[query] . x[key]
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dpt = sc, dpn = sc;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float4 xa = ld4(xrow + 4 * f), ga = ld4(grow + 4 * f);
          sc = mfma16(xa.x, bx[f].x, sc); dpt = mfma16(xa.x, bg[f].x, dpt); dpn = mfma16(ga.x, bx[f].x, dpn);
          sc = mfma16(xa.y, bx[f].y, sc); dpt = mfma16(xa.y, bg[f].y, dpt); dpn = mfma16(ga.y, bx[f].y, dpn);
          sc = mfma16(xa.z, bx[f].z, sc); dpt = mfma16(xa.z, bg[f].z, dpt); dpn = mfma16(ga.z, bx[f].z, dpn);
          sc = mfma16(xa.w, bx[f].w, sc); dpt = mfma16(xa.w, bg[f].w, dpt); dpn = mfma16(ga.w, bx[f].w, dpn);
        }
        const float4 l4 = ld4(st_l + t * 16 + 4 * q), t4 = ld4(st_t + t * 16 + 4 * q);
        const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, tq[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int pr = t * 16 + 4 * q + r;  // the partner's row in the tile
          // own token as query, partner as key
          float pa = __builtin_amdgcn_exp2f(fmaf(sc[r], c1, -l_own));
          if (LAST) pa = (k0 + pr < L) ? pa : 0.f;
          const float dsa = (scale * pa) * (dpt[r] - t_own);
          // own token as key, partner as query (lse = +inf past L: 0)
          const float pb = __builtin_amdgcn_exp2f(fmaf(sc[r], c1, -lq[r]));
          const float dsab = dsa + (scale * pb) * (dpn[r] - tq[r]);
          const float* xr = xs + pr * LDX + i;
          const float* gr = das + pr * LDX + i;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            acc[c] = mfma16(dsab, xr[c * 16], acc[c]);   // dq + dk: (dS[own][partner] + dS[partner][own]) x[partner]
            acv[c] = mfma16(pb, gr[c * 16], acv[c]);     // dv: P[partner][own] dA[partner]
          }
        }
      };
      const int nb = min(SRL_NT, (L - k0 + 15) / 16);  // 16-token blocks of this tile that hold a token (>= 1)
      const bool ragged = k0 + nb * 16 > L;            // the last of them holds padding keys (the last tile only)
#pragma nounroll
      for (int t = 0; t < nb - 1; ++t) partner_block(t, std::false_type{});
      if (ragged) partner_block(nb - 1, std::true_type{});
      else partner_block(nb - 1, std::false_type{});
    }
    // the other buffer was last read in the previous trip, which every wave left through the barrier below
    if (kt + 1 < ntile) tile_store(smem + ((kt + 1) & 1) * BUF, k0 + SRL_TK);
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = q0 + 4 * q + r;
      if (row < L) dx[base + (int64_t)row * d + c * 16 + i] += acc[c][r] + acv[c][r];
    }
  }
}

// every other head depth (and ULTR_SR_SCALAR_ATTN=1): the same two-role walk, scalar.  One workgroup = 4 waves x 4 own tokens of one
// (list, head); partner tiles of 64 rows of x and dA with their lse and t, one partner per lane.  Per own token the wave forms, for
// its lane's partner, S, dP^T and dP as three dot products over the head depth, then dS[own][partner] + dS[partner][own] and
// P[partner][own]; the two vectors go through LDS and lanes c < dh add their column of the own token's output row, which lives in LDS.
// LDS: (2 x 64 + 2 x 16) (dh + 1) + 16 dh + 2 x 64 + 4 x 2 x 64 floats - a function of dh alone.
size_t srs_bwd_lds_bytes(int dh) {
  return ((size_t)(2 * SRS_TK + 2 * SRS_QB) * (dh + 1) + (size_t)SRS_QB * dh + 2 * SRS_TK + 8 * SRS_TK) * sizeof(float);
}

__global__ __launch_bounds__(256) void sr_attn_bwd_long_scalar_kernel(const float* __restrict__ x, const float* __restrict__ dA,
                                                                      const float* __restrict__ lse, const float* __restrict__ tws, int batch,
                                                                      int L, int d, int dh, int nqb, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = dh + 1;
  float* ks = smem;                   // [64][dh + 1] partner x, zero rows past L
  float* gs = ks + SRS_TK * ldx;      // [64][dh + 1] partner dA
  float* xo = gs + SRS_TK * ldx;      // [16][dh + 1] own x
  float* go = xo + SRS_QB * ldx;      // [16][dh + 1] own dA
  float* os = go + SRS_QB * ldx;      // [16][dh]     own output rows
  float* pl = os + SRS_QB * dh;       // [64] partner lse (+inf past L)
  float* pt = pl + SRS_TK;            // [64] partner t
  float* ps = pt + SRS_TK;            // [4 waves][2][64] dS sums and probabilities of the wave's current own token
  const int qb = blockIdx.x % nqb, b = blockIdx.z * (gridDim.x / nqb) + blockIdx.x / nqb, h = blockIdx.y, H = gridDim.y;
  if (b >= batch) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = qb * SRS_QB;
  const int64_t base = (int64_t)b * L * d + h * dh;
  const int64_t sbase = (int64_t)b * L;
  for (int e = tid; e < SRS_QB * dh; e += 256) {
    const int r = e / dh, c = e - r * dh;
    const bool ok = q0 + r < L;
    xo[r * ldx + c] = ok ? x[base + (int64_t)(q0 + r) * d + c] : 0.f;
    go[r * ldx + c] = ok ? dA[base + (int64_t)(q0 + r) * d + c] : 0.f;
    os[e] = 0.f;
  }
  const float scale = 1.0f / sqrtf((float)dh);
  float l_own[SRS_QW], t_own[SRS_QW];  // wave-uniform
#pragma unroll
  for (int u = 0; u < SRS_QW; ++u) {
    const int row = q0 + wave * SRS_QW + u;
    l_own[u] = row < L ? lse[(sbase + row) * H + h] : INFINITY;
    t_own[u] = row < L ? tws[(sbase + row) * H + h] : 0.f;
  }
  float* pw = ps + wave * 2 * SRS_TK;
  for (int k0 = 0; k0 < L; k0 += SRS_TK) {
    __syncthreads();  // the previous tile's readers are done (first trip: nothing to wait for)
    for (int e = tid; e < SRS_TK * dh; e += 256) {
      const int r = e / dh, c = e - r * dh;
      const bool ok = k0 + r < L;
      ks[r * ldx + c] = ok ? x[base + (int64_t)(k0 + r) * d + c] : 0.f;
      gs[r * ldx + c] = ok ? dA[base + (int64_t)(k0 + r) * d + c] : 0.f;
    }
    if (tid < SRS_TK) {
      const bool ok = k0 + tid < L;
      pl[tid] = ok ? lse[(sbase + k0 + tid) * H + h] : INFINITY;
      pt[tid] = ok ? tws[(sbase + k0 + tid) * H + h] : 0.f;
    }
    __syncthreads();
    const float lp = pl[lane], tp = pt[lane];
#pragma unroll
    for (int u = 0; u < SRS_QW; ++u) {
      const int qi = wave * SRS_QW + u;
      if (q0 + qi < L) {  // wave-uniform
        float s = 0.f, dpt = 0.f, dpn = 0.f;
        for (int c = 0; c < dh; ++c) {
          const float xk = ks[lane * ldx + c], xq = xo[qi * ldx + c];
          s += xq * xk;                      // S[own][partner] = S[partner][own]
          dpt += go[qi * ldx + c] * xk;      // dP[query own][key partner]
          dpn += gs[lane * ldx + c] * xq;    // dP[query partner][key own]
        }
        const float pa = (k0 + lane < L) ? expf(s * scale - l_own[u]) : 0.f;  // own as query; padding keys masked
        const float pb = expf(s * scale - lp);                               // own as key; a padding query has lse = +inf: 0
        pw[lane] = scale * (pa * (dpt - t_own[u]) + pb * (dpn - tp));
        pw[SRS_TK + lane] = pb;
        __builtin_amdgcn_wave_barrier();
        for (int c = lane; c < dh; c += 64) {
          float a = os[qi * dh + c];
          for (int j = 0; j < SRS_TK; ++j) a += pw[j] * ks[j * ldx + c] + pw[SRS_TK + j] * gs[j * ldx + c];
          os[qi * dh + c] = a;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
#pragma unroll
  for (int u = 0; u < SRS_QW; ++u) {
    const int row = q0 + wave * SRS_QW + u;
    if (row < L)  // the wave reads the output rows it wrote itself
      for (int c = lane; c < dh; c += 64) dx[base + (int64_t)row * d + c] += os[(wave * SRS_QW + u) * dh + c];
  }
}

template <int DH>
int srl_launch_bwd_mfma(const SrAttnShape& p, const float* x, const float* dA, const float* Aout, const float* lse, int batch, int L, float* dx,
                        float* tws, hipStream_t st) {
  SrlGrid g;
  const int rc = srl_grid(batch, L, p.H, SRL_QB, SRL_NTHR, &g);
  if (rc != 0) return rc;
  const size_t lds = (size_t)2 * (2 * SRL_TK * (DH + 4) + 2 * SRL_TK) * sizeof(float);
  const int lrc = set_dyn_lds(sr_attn_bwd_long_kernel<DH>, lds);
  if (lrc != 0) return lrc;  // (before the first launch: a refusal leaves nothing launched)
  const int64_t T = (int64_t)batch * L, nthr = T * p.H * (DH / 4);
  hipLaunchKernelGGL(sr_attn_t_kernel<DH>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, dA, Aout, T, p.d, DH, p.H, tws);
  hipLaunchKernelGGL(sr_attn_bwd_long_kernel<DH>, g.grid, dim3(SRL_NTHR), lds, st, x, dA, lse, tws, batch, L, p.d, g.nqb, dx);
  return 0;
}

}  // namespace

bool sr_attn_long_scalar_fits(int dh) { return srs_lds_bytes(dh) <= 160 * 1024; }

int sr_attn_forward_long(const SrAttnShape& s, bool mfma, const float* x, int batch, int L, float* A, float* lse, hipStream_t st) {
  if (mfma) {
    if (s.dh == 16) return srl_launch_mfma<16>(s, x, batch, L, A, lse, st);
    if (s.dh == 32) return srl_launch_mfma<32>(s, x, batch, L, A, lse, st);
    if (s.dh == 64) return srl_launch_mfma<64>(s, x, batch, L, A, lse, st);
    return ULTR_E_UNSUPPORTED;
  }
  SrlGrid g;
  int rc = srl_grid(batch, L, s.H, SRS_QB, 256, &g);
  if (rc != 0) return rc;
  const size_t lds = srs_lds_bytes(s.dh);
  rc = set_dyn_lds(sr_attn_fwd_long_scalar_kernel, lds);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(sr_attn_fwd_long_scalar_kernel, g.grid, dim3(256), lds, st, x, batch, L, s.d, s.dh, g.nqb, A, lse);
  return 0;
}

bool sr_attn_bwd_long_scalar_fits(int dh) { return srs_bwd_lds_bytes(dh) <= 160 * 1024; }

int sr_attn_backward_long(const SrAttnShape& s, bool mfma, const float* x, const float* dA, const float* Aout, const float* lse, int batch, int L,
                          float* dx, float* tws, hipStream_t st) {
  if (tws == nullptr || lse == nullptr) return ULTR_E_WORKSPACE;
  if (mfma) {
    if (s.dh == 16) return srl_launch_bwd_mfma<16>(s, x, dA, Aout, lse, batch, L, dx, tws, st);
    if (s.dh == 32) return srl_launch_bwd_mfma<32>(s, x, dA, Aout, lse, batch, L, dx, tws, st);
    if (s.dh == 64) return srl_launch_bwd_mfma<64>(s, x, dA, Aout, lse, batch, L, dx, tws, st);
    return ULTR_E_UNSUPPORTED;
  }
  SrlGrid g;
  int rc = srl_grid(batch, L, s.H, SRS_QB, 256, &g);
  if (rc != 0) return rc;
  const size_t lds = srs_bwd_lds_bytes(s.dh);
  rc = set_dyn_lds(sr_attn_bwd_long_scalar_kernel, lds);
  if (rc != 0) return rc;
  const int64_t T = (int64_t)batch * L;
  hipLaunchKernelGGL(sr_attn_t_kernel<0>, dim3((unsigned)((T * s.H + 255) / 256)), dim3(256), 0, st, dA, Aout, T, s.d, s.dh, s.H, tws);
  hipLaunchKernelGGL(sr_attn_bwd_long_scalar_kernel, g.grid, dim3(256), lds, st, x, dA, lse, tws, batch, L, s.d, s.dh, g.nqb, dx);
  return 0;
}
