// ultr_plrank.hip — gfx950 loss kernel of PLRank, the Plackett-Luce policy gradient of the expected DCG@K   
//
// The ranker's scores are a Plackett-Luce policy; the kernel follows the sampled, low-variance gradient of PL-Rank (Oosterhuis, SIGIR
// 2021: PL-Rank-2 evaluated in PL-Rank-3's linear time) of  E[sum_{k < K} theta_k rho_{y_k}],  theta_k = 1 / log2(k + 2),  with the
// IPW-weighted clicks rho_l = w_l gain(y_l) as relevance estimates.  The project's own algorithm: the reference has no such class.
//
// Per list (one workgroup, LOSS_JW waves): wave 0 stages s (PADs as -inf), rho, validity and e = exp(s - max over valid s) into LDS.
// Then wave jw takes the samples n = jw, jw + LOSS_JW, ... in ascending order.  Per sample:
//   the exponential race of ultr_rank.h at tau = 1 (wave_rank_keys; uniform of position l = philox_word(key(seed, step), b, n, l,
//   PLRANK_TAG)) and the rank by counting into the wave's perm: the n_pos drawn documents by descending key, then the documents of
//   fp32 probability 0 and the PADs in index order;  K_eff = min(K, n_pos);
//   two backward wave scans over the ranks, in trips of 64 lanes from the last trip to the first:
//     Z_k  = sum of e over the valid documents at ranks >= k          (positives only)
//     FR_k = sum_{x = k}^{K_eff - 1} theta_x rho_{y_x},  FR_{K_eff} = 0
//   two forward wave scans:  RI_i = sum_{k <= i} FR_k / Z_k,  DR_i = sum_{k <= i} theta_k / Z_k  (terms at k >= K_eff are 0, so the
//   scan value at rank r is the one at i = min(r, K_eff - 1));
//   the lane of rank r adds  g_d = [r < K_eff] FR_{r + 1} + e_d (rho_d DR_i - RI_i)  to the wave's private acc[d], d = perm[r] valid
//   (perm is a permutation: no two lanes meet).
// The list's wave 0 folds the LOSS_JW partials in the order 0 .. LOSS_JW - 1:  dscores[b, d] = -(1 / N) sum_n g_d,  tail
// [-(1 / N) sum_n FR_0, 1, 0, 0, zeros] (D counts lists; the update launch divides).  No atomics: same inputs, seed, step - same bits.
//
// Numerics.  Every output is homogeneous of degree 0 in e, so the kernel works with e' = e * exp(PLRANK_SHIFT): a drawn document has
// log p >= ln 2^-150, hence Z_k >= e^-104 for k < K_eff and 1 / Z_k would overflow fp32 unscaled (and the small e would be
// subnormal, a few bits each).  With the shift Z', 1 / Z', FR / Z' and the scans stay normal numbers.  e' itself is kept in two
// factors, ea = exp(max(t, PLRANK_SPLIT)) and eb = exp(min(t - PLRANK_SPLIT, 0)), t = s - max + PLRANK_SHIFT: g = (ea A) eb is right
// to fp32 precision wherever g itself is a normal fp32 number, down to documents e^-230 below the best one (eb = 1 for all others).
// s - max and the shift are formed as exact two-term sums (the rounding of a difference near 100 is 4e-6 of e): the low terms
// enter as the factor 1 + lo.
// Lists up to PlRankLds: 465 documents in the CU's 160 KiB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"
#include "ultr_rank.h"

#define PLRANK_TAG 0x504C524Bu  // "PLRK": the race stream of the sampled rankings (no other kernel's tag)
#define PLRANK_SHIFT 64.0f
#define PLRANK_SPLIT -80.0f

// inclusive sums over the lanes at and after this one / at and before this one, two values at once (fixed order)
__device__ __forceinline__ void wave_suffix2(float& a, float& b, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ua = __shfl_down(a, o), ub = __shfl_down(b, o);
    if (lane + o < 64) {
      a += ua;
      b += ub;
    }
  }
}
__device__ __forceinline__ void wave_prefix2(float& a, float& b, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ua = __shfl_up(a, o), ub = __shfl_up(b, o);
    if (lane >= o) {
      a += ua;
      b += ub;
    }
  }
}

__global__ __launch_bounds__(LPW * LOSS_JW * 64) void plrank_kernel(const float* __restrict__ scores, const float* __restrict__ labels,
                                                                  const float* __restrict__ pw, const float* __restrict__ ipw_table,
                                                                  int n_ipw, const int32_t* __restrict__ docids, int64_t n_docs, int K,
                                                                  int N, int exp2_gain, uint64_t seed, uint64_t step, int B, int L,
                                                                  float* __restrict__ dscores, int32_t* __restrict__ perm_out,
                                                                  float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const PlRankLds lay(L);
  const ListWave at = list_wave(L);
  const int lane = at.lane, lw = at.lw, jw = at.jw, b = at.b;
  const int wv = lw * LOSS_JW + jw;
  float* sm_tail = smem + lay.tail;
  float* mt = sm_tail + lw * tail;
  float* sm_d = smem + lay.d;
  float* ms = smem + lay.s + lw * L;
  float* rho = smem + lay.rho + lw * L;
  float* ea = smem + lay.ea + lw * L;
  float* eb = smem + lay.eb + lw * L;
  int* mv = reinterpret_cast<int*>(smem + lay.v) + lw * L;
  int* hdr = reinterpret_cast<int*>(smem + lay.hdr) + lw;
  float* red = smem + lay.red + lw * LOSS_JW;
  unsigned* key = reinterpret_cast<unsigned*>(smem + lay.key) + (size_t)wv * L;
  int* perm = reinterpret_cast<int*>(smem + lay.perm) + (size_t)wv * L;
  float* zk = smem + lay.z + (size_t)wv * L;
  float* fr = smem + lay.fr + (size_t)wv * (L + 1);
  float* acc = smem + lay.acc + (size_t)wv * L;

  for (int t = threadIdx.x; t < L; t += blockDim.x) sm_d[t] = 1.0f / log2f((float)t + 2.0f);
  for (int l = lane; l < L; l += 64) acc[l] = 0.f;
  if (jw == 0) {
    for (int t = lane; t < tail; t += 64) mt[t] = 0.f;
    if (b < B) {
      float mx = -INFINITY;
      int nv = 0;
      for (int l = lane; l < L; l += 64) {
        const int64_t id = docids[(int64_t)l * B + b];
        const bool ok = id >= 0 && id < n_docs;
        const float s = ok ? scores[(int64_t)b * L + l] : -INFINITY;
        ms[l] = s;
        mv[l] = ok ? 1 : 0;
        mx = fmaxf(mx, s);
        nv += ok ? 1 : 0;
      }
      mx = wave_max(mx);
      nv = (int)wave_sum((float)nv);  // (exact: at most 465)
      for (int l = lane; l < L; l += 64) {
        float r = 0.f, a = 0.f, c = 0.f;
        if (mv[l]) {
          const float y = labels[(int64_t)l * B + b];
          const float w = pw != nullptr ? pw[(int64_t)b * L + l] : (ipw_table != nullptr ? ipw_table[l < n_ipw ? l : n_ipw - 1] : 1.0f);
          r = w * (exp2_gain ? exp2f(y) - 1.0f : y);
          const float s = ms[l];
          // s - mx = hi + lo and hi + PLRANK_SHIFT = t + lo2, both exactly (two-term sums)
          const float hi = s - mx;
          const float bb = hi - s;
          float lo = (s - (hi - bb)) - (mx + bb);
          const float t = hi + PLRANK_SHIFT;
          const float tb = t - hi;
          lo += (hi - (t - tb)) + (PLRANK_SHIFT - tb);
          if (!(hi > -INFINITY)) lo = 0.f;
          a = expf(fmaxf(t, PLRANK_SPLIT)) * (1.0f + lo);
          c = expf(fminf(t - PLRANK_SPLIT, 0.f));
        }
        rho[l] = r;
        ea[l] = a;
        eb[l] = c;
      }
      if (lane == 0) hdr[0] = nv;
    }
  }
  __syncthreads();  // the staged list is visible to its other waves

  float rsum = 0.f;  // this wave's sum of FR_0 over its samples (wave-uniform)
  if (b < B) {
    const Philox rng = philox_step_key(seed, step);
    const int n_valid = hdr[0];
    const int trips = (L + 63) >> 6;
    for (int n = jw; n < N; n += LOSS_JW) {
      // the draw: race keys, the drawn count, the order
      if (n_valid > 0) {
        wave_rank_keys(ms, L, true, 1.0f, rng, (uint32_t)b, (uint32_t)n, PLRANK_TAG, key, lane);
      } else {  // nothing to draw: every key ties, the order is the index order
        for (int l = lane; l < L; l += 64) key[l] = 0u;
        wave_lds_sync();
      }
      int n_pos = 0;
      for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        n_pos += __popcll(__ballot(l < L && key[l] != 0u));
      }
      wave_rank_by_count(key, L, perm, lane);
      wave_lds_sync();
      if (perm_out != nullptr) {
        int32_t* po = perm_out + ((int64_t)b * N + n) * L;
        for (int r = lane; r < L; r += 64) po[r] = perm[r];
      }
      const int k_eff = K < n_pos ? K : n_pos;
      if (k_eff > 0) {
        // backward scans: Z_k and FR_k, the carry holds the later trips' totals
        float cz = 0.f, cf = 0.f;
        for (int t = trips - 1; t >= 0; --t) {
          const int r = t * 64 + lane;
          const int d = r < L ? perm[r] : 0;
          float z = r < L ? ea[d] * eb[d] : 0.f;
          float f = r < k_eff ? sm_d[r] * rho[d] : 0.f;
          wave_suffix2(z, f, lane);
          z += cz;
          f += cf;
          if (r < L) {
            zk[r] = z;
            fr[r] = f;
          }
          cz = __shfl(z, 0);
          cf = __shfl(f, 0);
        }
        if (lane == 0) fr[L] = 0.f;
        rsum += cf;  // FR_0
        wave_lds_sync();
        // forward scans RI and DR, then each rank's document takes its g
        float cri = 0.f, cdr = 0.f;
        for (int t = 0; t < trips; ++t) {
          const int r = t * 64 + lane;
          const bool in = r < k_eff;
          const float z = in ? zk[r] : 1.0f;
          float ri = in ? fr[r] / z : 0.f;
          float dr = in ? sm_d[r] / z : 0.f;
          wave_prefix2(ri, dr, lane);
          ri += cri;
          dr += cdr;
          if (r < L) {
            const int d = perm[r];
            if (mv[d]) acc[d] += (in ? fr[r + 1] : 0.f) + (ea[d] * (rho[d] * dr - ri)) * eb[d];
          }
          cri = __shfl(ri, 63);
          cdr = __shfl(dr, 63);
        }
      }
      wave_lds_sync();  // the next sample overwrites key, perm, zk, fr
    }
    if (lane == 0) red[jw] = rsum;
  }
  __syncthreads();
  if (b < B && jw == 0) {
    const float fn = (float)N;
    const float* acc0 = smem + lay.acc + (size_t)(lw * LOSS_JW) * L;
    for (int d = lane; d < L; d += 64) {
      float g = acc0[d];
#pragma unroll
      for (int w = 1; w < LOSS_JW; ++w) g += acc0[(size_t)w * L + d];
      dscores[(int64_t)b * L + d] = 0.f - g / fn;
    }
    if (lane == 0) {
      float r = red[0];
#pragma unroll
      for (int w = 1; w < LOSS_JW; ++w) r += red[w];
      mt[0] = 0.f - r / fn;
      mt[1] = 1.0f;  // D counts lists
    }
  }
  store_wg_tail(sm_tail, tail, part + (int64_t)blockIdx.x * tail);
}

extern "C" int ultr_plrank_loss(const float* scores, const float* labels, const float* pw, const float* ipw_table, int32_t n_ipw,
                                const int32_t* docids, int64_t n_docs, int32_t cutoff, int32_t n_samples, int32_t gain, uint64_t rng_seed,
                                uint64_t rng_step, int32_t batch, int32_t list_size, float* dscores, int32_t* perm_out, void* loss_ws,
                                void* stream) {
  if (!scores || !labels || !docids || !dscores || !loss_ws || batch <= 0 || list_size <= 0 || n_docs < 0 || cutoff < 0 ||
      n_samples < 1 || n_samples > ULTR_PLRANK_MAX_SAMPLES || (gain != ULTR_PLRANK_GAIN_LINEAR && gain != ULTR_PLRANK_GAIN_EXP2) ||
      (ipw_table && n_ipw <= 0))
    return ULTR_E_BADARG;
  const int K = (cutoff == 0 || cutoff > list_size) ? list_size : cutoff;
  return launch_list_loss(plrank_kernel, LPW * LOSS_JW * 64, PlRankLds(list_size).bytes, PlRankLds::limit, batch, stream, scores, labels,
                          pw, ipw_table, (int)n_ipw, docids, n_docs, K, (int)n_samples, (int)gain, rng_seed, rng_step, batch, list_size,
                          dscores, perm_out, (float*)loss_ws);
}
