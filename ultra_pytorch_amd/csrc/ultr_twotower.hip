// ultr_twotower.hip — gfx950 loss kernel of TwoTower, the pointwise two-tower click model   
//
// A relevance tower (the ranking model's score s) and an observation tower (one logit theta_l per position), trained jointly by
// maximum likelihood on the clicks c = min(label, 1):  P(click) = sigmoid(s) sigmoid(theta_l)  (product)  or  sigmoid(s + theta_l)
// (sum);  element loss  -c log p - (1 - c) log(1 - p),  summed over the positions of a list, mean over the lists (D = lists).
// The project's own algorithm: the likelihood twin of RegressionEM (regem_kernel) and the pointwise twin of DLA (dla_loss_kernel).
//
// One wavefront per list, lanes over positions in trips of 64; nothing is staged, only the step tail sits in LDS.  The kernel emits
// dscores = d l / d s (x D) and the tail [sum l, 1 per list, 0, 0, sum_b d l / d theta_l at ULTR_TAIL_FIXED + l]; the update launch
// divides by D and steps theta (update_body, ultr_update.hip).  No atomics.
//
// Numerics - every quantity is a sum of positives or a product, nothing is formed as 1 - (something near 1):
//   e_x = exp(-|x|);  sigmoid(|x|) = 1 / (1 + e_x),  sigmoid(-|x|) = e_x / (1 + e_x);  log sigmoid(x) = min(x, 0) - log1p(e_x)
//   product:  log p = log sigmoid(s) + log sigmoid(theta);  1 - p = q = sigmoid(-s) + sigmoid(s) sigmoid(-theta);
//             log(1 - p) = log1p(-p) where p < 0.5, log q otherwise;  r = (1 - c) p / q - c;
//             d l / d s = sigmoid(-s) r,  d l / d theta = sigmoid(-theta) r.
//     Where both towers saturate high, q ~ e^-s + e^-theta underflows in fp32 (from about 88) although log q and the gradients are of
//     order 1 .. 100: the common factor e^-t, t = max(0, min(s, theta)), is taken out of sigmoid(-s), sigmoid(-theta) and q - the
//     numerators become exp(t - x) - so  log q = log q' - t  and  sigmoid(-s) p / q = sigmoid'(-s) p / q'.  t = 0 (a tower at or
//     below 0) leaves exactly the forms above.
//   sum:      BCE-with-logits of z = s + theta as regem_kernel writes it, d l / d s = d l / d theta = sigmoid(z) - c.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"

struct TowerTerm {
  float loss, g_s, g_theta;  // the element loss, d l / d s, d l / d theta
};

// one tower's logit x: sigmoid(x), sigmoid(-x) scaled by e^t (t <= max(x, 0)), log sigmoid(x)
struct Tower {
  float sig, nsig_t, nsig, logsig;
};
__device__ __forceinline__ Tower tower_of(float x, float t) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  Tower w;
  w.sig = (x >= 0.f) ? r : e * r;
  w.nsig = (x >= 0.f) ? e * r : r;
  w.nsig_t = (x > 0.f) ? expf(t - x) * r : r;  // t == 0: sigmoid(-x) itself
  w.logsig = fminf(x, 0.f) - log1pf(e);
  return w;
}

__device__ __forceinline__ TowerTerm twotower_product(float s, float th, float c) {
  const float t = fmaxf(0.f, fminf(s, th));
  const Tower a = tower_of(s, t), b = tower_of(th, t);
  const float p = a.sig * b.sig;
  const float q = a.nsig_t + a.sig * b.nsig_t;  // (1 - p) e^t: a sum of positives, at least 0.25
  const float log_p = a.logsig + b.logsig;
  const float log_1mp = (p < 0.5f) ? log1pf(-p) : logf(q) - t;
  // c == 0 / c == 1 drop their term instead of multiplying it by 0: log p is -inf where p underflows
  const float pq = (c < 1.0f) ? (1.0f - c) * (p / q) : 0.f;
  TowerTerm o;
  o.loss = ((c > 0.f) ? -c * log_p : 0.f) + ((c < 1.0f) ? -(1.0f - c) * log_1mp : 0.f);
  o.g_s = a.nsig_t * pq - a.nsig * c;
  o.g_theta = b.nsig_t * pq - b.nsig * c;
  return o;
}

__device__ __forceinline__ TowerTerm twotower_sum(float s, float th, float c) {
  const float z = s + th;
  const float e = expf(-fabsf(z));
  const float r = 1.0f / (1.0f + e);
  TowerTerm o;
  o.loss = fmaxf(z, 0.f) - z * c + log1pf(e);  // BCEWithLogits element
  o.g_s = o.g_theta = ((z >= 0.f) ? r : e * r) - c;
  return o;
}

__global__ __launch_bounds__(LPW * 64) void twotower_kernel(const float* __restrict__ scores, const float* __restrict__ labels,
                                                           const float* __restrict__ bias_logits, int sum_form,
                                                           const int32_t* __restrict__ docids, int64_t n_docs, int B, int L,
                                                           float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const TwoTowerLds lay(L);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * LPW + wave;
  float* sm_tail = smem + lay.tail;
  float* mt = sm_tail + wave * tail;
  for (int t = lane; t < tail; t += 64) mt[t] = 0.f;
  if (b < B) {
    float lsum = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float s = scores[(int64_t)b * L + l];
      const float c = fminf(labels[(int64_t)l * B + b], 1.0f);
      const float th = bias_logits[l];
      bool live = true;
      if (docids != nullptr) {
        const int64_t id = docids[(int64_t)l * B + b];
        live = id >= 0 && id < n_docs;
      }
      TowerTerm o = sum_form ? twotower_sum(s, th, c) : twotower_product(s, th, c);
      if (!live) o.loss = o.g_s = o.g_theta = 0.f;  // a PAD: nothing to the loss, to dscores, to theta's gradient
      lsum += o.loss;
      dscores[(int64_t)b * L + l] = o.g_s;  // x D
      mt[ULTR_TAIL_FIXED + l] = o.g_theta;
    }
    lsum = wave_sum(lsum);
    if (lane == 0) {
      mt[0] = lsum;
      mt[1] = 1.0f;  // D counts lists
    }
  }
  store_wg_tail(sm_tail, tail, part + (int64_t)blockIdx.x * tail);
}

extern "C" int ultr_twotower_loss(const float* scores, const float* labels, const float* bias_logits, int32_t combination,
                                  const int32_t* docids, int64_t n_docs, int32_t batch, int32_t list_size, float* dscores, void* loss_ws,
                                  void* stream) {
  if (!scores || !labels || !bias_logits || !dscores || !loss_ws || batch <= 0 || list_size <= 0 ||
      (combination != 0 && combination != ULTR_TWOTOWER_SUM) || (docids && n_docs < 0))
    return ULTR_E_BADARG;
  return launch_list_loss(twotower_kernel, LPW * 64, TwoTowerLds(list_size).bytes, TwoTowerLds::limit, batch, stream, scores, labels,
                          bias_logits, (int)combination, docids, n_docs, batch, list_size, dscores, (float*)loss_ws);
}
