// ultr_affine.hip — gfx950 loss kernel of AffineRank, the listwise softmax loss under the affine correction of trust bias   
//
// Under trust bias a click at rank k on a document of relevance gamma has probability alpha_k gamma + beta_k with beta_k > 0: no
// inverse propensity weight is unbiased, the affine estimate (c - beta_k) / alpha_k is (Agarwal et al. 2019; Vardasbi et al. 2020).
// Per list, with c = labels[l, b] as it is, k = min(l, n_aff - 1), live = no docids or 0 <= docids[l, b] < n_docs:
//   w_l = live ? (c - beta_k) / alpha_k : 0         every live position, clicked or not; negative wherever c < beta_k
//   loss_b = sum_l w_l (lse - s_l)                   the softmax over all L positions (a PAD stays in the denominator, as in
//                                                    softmax_ce_kernel)
//   dscores[b, l] = softmax_l W_b - w_l              W_b = sum_l w_l in double, rounded once (softmax_ce_dscore, ultr_device.h)
// Nothing assumes a sign: w_l, W_b and loss_b may be negative or zero.  The step tail is [sum_b loss_b, 1 per list, 0, 0, zeros]: D
// counts lists, the update launch divides - W_b is no normaliser here, it may vanish.
//
// One wavefront per list, lanes over positions in trips of 64, scores and weights staged in LDS (SoftmaxLds under the kernel's own
// name).  No atomics: the same inputs give the same bits.
//
// Numerics.  s - max is kept as an exact two-term sum hi + lo and exp(s - max) = exp(hi) (1 + lo): at score differences of 64 .. 128 the
// rounding of the difference alone is 4e-6 of the exponential.  lse - s is formed as (max - s) + log(sum), not from the rounded lse.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"

// exp(s - mx) from the exact difference: hi = fl(s - mx), lo = (s - mx) - hi (two-sum), exp(hi + lo) = exp(hi) (1 + lo) to O(lo^2)
__device__ __forceinline__ float exp_diff(float s, float mx) {
  const float nb = -mx;
  const float hi = s + nb;
  const float bb = hi - s;
  const float lo = (s - (hi - bb)) + (nb - bb);
  const float e = expf(hi);
  return (hi > -INFINITY) ? fmaf(e, lo, e) : 0.f;  // (s = -inf: lo is NaN, the exponential is 0)
}

__global__ __launch_bounds__(LPW * 64) void affine_loss_kernel(const float* __restrict__ scores, const float* __restrict__ labels,
                                                              const float* __restrict__ alpha, const float* __restrict__ beta, int n_aff,
                                                              const int32_t* __restrict__ docids, int64_t n_docs, int B, int L,
                                                              float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const AffineLds lay(L);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * LPW + wave;
  float* sm_tail = smem + lay.tail;
  float* ms = smem + lay.s + wave * L;
  float* mw = smem + lay.w + wave * L;
  float* mt = sm_tail + wave * tail;
  for (int t = lane; t < tail; t += 64) mt[t] = 0.f;
  if (b < B) {
    float mx = -INFINITY;
    double Wd = 0.0;
    for (int l = lane; l < L; l += 64) {
      const float s = scores[(int64_t)b * L + l];
      const float c = labels[(int64_t)l * B + b];
      const int k = l < n_aff ? l : n_aff - 1;
      bool live = true;
      if (docids != nullptr) {
        const int64_t id = docids[(int64_t)l * B + b];
        live = id >= 0 && id < n_docs;
      }
      const float w = live ? (c - beta[k]) / alpha[k] : 0.f;
      ms[l] = s;
      mw[l] = w;
      mx = fmaxf(mx, s);
      Wd += (double)w;
    }
    mx = wave_max(mx);
    const float W = (float)wave_sum_d(Wd);  // the weight sum rounded ONCE
    float se = 0.f;
    for (int l = lane; l < L; l += 64) se += exp_diff(ms[l], mx);
    se = wave_sum(se);
    const float lg = logf(se);
    float lb = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float s = ms[l], w = mw[l];
      lb += w * ((mx - s) + lg);  // -w log_softmax(s)
      dscores[(int64_t)b * L + l] = softmax_ce_dscore(exp_diff(s, mx), se, W, w);  // x D
    }
    lb = wave_sum(lb);
    if (lane == 0) {
      mt[0] = lb;
      mt[1] = 1.0f;  // D counts lists
    }
  }
  store_wg_tail(sm_tail, tail, part + (int64_t)blockIdx.x * tail);
}

extern "C" int ultr_affine_loss(const float* scores, const float* labels, const float* alpha, const float* beta, int32_t n_aff,
                                const int32_t* docids, int64_t n_docs, int32_t batch, int32_t list_size, float* dscores, void* loss_ws,
                                void* stream) {
  if (!scores || !labels || !alpha || !beta || !dscores || !loss_ws || batch <= 0 || list_size <= 0 || n_aff <= 0 ||
      (docids && n_docs < 0))
    return ULTR_E_BADARG;
  return launch_list_loss(affine_loss_kernel, LPW * 64, AffineLds(list_size).bytes, AffineLds::limit, batch, stream, scores, labels,
                          alpha, beta, (int)n_aff, docids, n_docs, batch, list_size, dscores, (float*)loss_ws);
}
