// ultr_pdgd.hip — gfx950 loss kernel of PDGD, Pairwise Differentiable Gradient Descent   (reference pdgd.py:107-205)
//
// One list per workgroup of four wavefronts (L <= PDGD_MAX_L).  Per list:
//   m = max_j s_j over ALL positions (PADs included), e_j = exp(tau (s_j - m)) in fp32, e_j = 0 for a PAD (docid == n_docs)
//   at j < cutoff ONLY (pdgd.py:120-126 zeroes PADs in range(rank_list_size): a PAD past the cutoff keeps its exp-score);
//   D_p = sum_{q >= p} e_q, summed from the end one position at a time as numpy's cumsum of the reversed row does.
// The pairs (pdgd.py:138-172): l valid, l < cutoff, label_l > 0; k in 0 .. l+1, k < cutoff, k valid, label_k < label_l.
// Swapping k and l (a = min, b = max) changes only the suffix sums D_p for a < p <= b, to F_p, so the flipped list's sum
// of logs minus the original's is the local
//   delta = sum_{a < p <= b} lg(F_p) - lg(D_p),   lg(x) = x > 0 ? log x : 0   (the `where=denominators > 0`),
// each term taken as log1p((F_p - D_p) / D_p) where both sides are positive: more accurate than the reference's difference
// of two full fp32 sums.  w = 1 / (1 + exp(min(delta, 20))) is a constant.  The loss term is -w e^{s_l} / (e^{s_l} + e^{s_k}) on
// the RAW scores (no tau, no shift), and its gradient is autograd's through that exact expression in fp32 (x = e^{s_l},
// y = e^{s_k}, v = x + y; the numerator's and the denominator's exp are separate nodes):
//   d s_l = -(w / v) x + (w ((x / v) / v)) x,   d s_k = (w ((x / v) / v)) y     (NaN where exp overflows, as there).
//
// Work split: the pair weights first, one wavefront per clicked row l and its lanes over k (a lane's delta loop runs |l - k|
// steps, so a row costs about l steps), into an LDS triangle of L (L + 3) / 2 floats; then one thread per position j sums
// its pairs' gradient terms from the stored weights - first those where it is l (in k order), then those where it is k
// (in l order).  Fixed summation orders and no atomics: the same inputs give bitwise-identical outputs.  The loss terms
// are counted by the l side and reduced in fixed order (wave DPP sums, then waves in index order).  Plain sum:
// tail[0] = loss, the update divides by nothing (ULTR_ALGO_PDGD: D = 1).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"

static_assert(ULTR_LOSS_LISTS_PER_WG == 1, "pdgd_loss_kernel writes one loss partial per list");

// delta of the flipped list, positions a < b swapped.  Only the suffix sums in (a, b] differ; the flipped ones are summed from
// the end exactly as the reference's cumsum of the flipped row sums them: F_b = D_{b+1} + e_a, F_p = F_{p+1} + e_p (forming
// D_p - e_b + e_a instead cancels catastrophically where e_b dominates the suffix and e_a has underflowed next to it).
__device__ __forceinline__ float pdgd_delta(const float* __restrict__ e, const float* __restrict__ D, int a, int b) {
  float f = D[b + 1] + e[a];
  float delta = 0.f;
  for (int p = b; p > a; --p) {
    if (p < b) f += e[p];
    const float d = D[p];
    if (d > 0.f && f > 0.f)
      delta += log1pf((f - d) / d);
    else
      delta += (f > 0.f ? logf(f) : 0.f) - (d > 0.f ? logf(d) : 0.f);
  }
  return delta;
}

__global__ __launch_bounds__(PDGD_THREADS) void pdgd_loss_kernel(const float* __restrict__ scores,
                                                                 const float* __restrict__ labels,
                                                                 const int32_t* __restrict__ docids, int64_t n_docs,
                                                                 float tau, int cutoff, int B, int L,
                                                                 float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PdgdLds lay(L);
  float* sm_s = smem + lay.s;
  float* sm_x = smem + lay.x;
  float* sm_y = smem + lay.y;
  float* sm_e = smem + lay.e;
  float* sm_D = smem + lay.D;
  int* sm_v = reinterpret_cast<int*>(smem + lay.v);
  float* sm_red = smem + lay.red;
  float* sm_w = smem + lay.w;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x;
  const int tail = (int)ultr_tail_len(L);
  const bool in = t < L;
  float s = -INFINITY;
  if (in) {
    s = scores[(int64_t)b * L + t];
    sm_s[t] = s;
    sm_x[t] = expf(s);
    sm_y[t] = labels[(int64_t)t * B + b];
    sm_v[t] = (int64_t)docids[(int64_t)t * B + b] != n_docs;
  }
  // m = max over the list: exact in any order
  float mx = s;
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) sm_red[wave] = mx;
  __syncthreads();
  mx = sm_red[0];
  for (int w = 1; w < PDGD_WAVES; ++w) mx = fmaxf(mx, sm_red[w]);
  if (in) sm_e[t] = (t < cutoff && !sm_v[t]) ? 0.f : expf(tau * (s - mx));
  __syncthreads();
  if (t == 0) {
    float acc = 0.f;
    sm_D[L] = 0.f;
    for (int p = L - 1; p >= 0; --p) {
      acc += sm_e[p];
      sm_D[p] = acc;
    }
  }
  __syncthreads();
  // pair weights: one wave per clicked row l, its lanes over k = 0 .. l+1 (a lane's delta loop runs l - k steps)
  for (int l = wave; l < cutoff; l += PDGD_WAVES) {
    const float yl = sm_y[l];
    if (!sm_v[l] || !(yl > 0.f)) continue;
    const int kend = min(l + 1, cutoff - 1);
    for (int k = lane; k <= kend; k += 64) {
      if (!sm_v[k] || !(sm_y[k] < yl)) continue;
      const float delta = (k < l) ? pdgd_delta(sm_e, sm_D, k, l) : pdgd_delta(sm_e, sm_D, l, k);
      sm_w[pdgd_row(l) + k] = 1.0f / (1.0f + expf(fminf(delta, 20.0f)));
    }
  }
  __syncthreads();
  // gradients: thread j sums the pairs where it is l (in k order), then those where it is k (in l order)
  float g = 0.f, li = 0.f;
  if (in && t < cutoff && sm_v[t]) {
    const float yj = sm_y[t];
    if (yj > 0.f) {
      const int kend = min(t + 1, cutoff - 1);
      const float x = sm_x[t];
      for (int k = 0; k <= kend; ++k) {
        if (!sm_v[k] || !(sm_y[k] < yj)) continue;
        const float w = sm_w[pdgd_row(t) + k];
        const float y = sm_x[k], v = x + y;
        li += (-x / v) * w;
        g += -(w / v) * x + (w * ((x / v) / v)) * x;
      }
    }
    const float y = sm_x[t];
    for (int l = max(t - 1, 0); l < cutoff; ++l) {
      const float yl = sm_y[l];
      if (!sm_v[l] || !(yl > 0.f) || !(yj < yl)) continue;
      const float w = sm_w[pdgd_row(l) + t];
      const float x = sm_x[l], v = x + y;
      g += (w * ((x / v) / v)) * y;
    }
  }
  if (in) dscores[(int64_t)b * L + t] = g;
  li = wave_sum(li);
  __syncthreads();  // (sm_red is reused)
  if (lane == 0) sm_red[wave] = li;
  __syncthreads();
  float* out = part + (int64_t)b * tail;
  for (int i = t; i < tail; i += blockDim.x) {
    float v = 0.f;
    if (i == 0)
      for (int w = 0; w < PDGD_WAVES; ++w) v += sm_red[w];
    out[i] = v;
  }
}

extern "C" int ultr_pdgd_loss(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, float tau,
                              int32_t cutoff, int32_t batch, int32_t list_size, float* dscores, void* loss_ws,
                              void* stream) {
  if (!scores || !labels || !docids || !dscores || !loss_ws || batch <= 0 || list_size <= 0 || cutoff < 0 || n_docs < 0)
    return ULTR_E_BADARG;
  if (list_size > PDGD_MAX_L) return ULTR_E_UNSUPPORTED;
  const int c = cutoff < list_size ? cutoff : list_size;
  return launch_list_loss(pdgd_loss_kernel, PDGD_THREADS, PdgdLds(list_size).bytes, PdgdLds::limit, batch, stream, scores, labels, docids,
                          n_docs, tau, c, batch, list_size, dscores, (float*)loss_ws);
}
