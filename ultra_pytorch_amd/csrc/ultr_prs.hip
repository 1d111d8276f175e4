// ultr_prs.hip — gfx950 loss kernel of PRSrank, the propensity-ratio-scored LambdaRank   (reference prs_rank.py:94-176, 207-251)
//
// The same decomposition as lambdarank_kernel (ultr_loss.hip), from the same pieces (ultr_listloss.h): one list per workgroup, wave 0
// of the list sorts by rank counting (ties broken by original index), then LOSS_JW waves each walk a slice of the partner positions c
// for every sorted position r; the two partial sums per position (d loss / d sorted score, loss) are combined in fixed order through LDS.
// Only the pairs i < j of the sorted order carry loss (triu(., 1)); the weights are indexed by PRESENTATION position and
// gathered into score order:  prs_ij = ipw_i * pw_j,  pw = ipw == 0 ? 0 : 1 / ipw  (use_non_clicked_data=True).  The ipw of a
// position is the table's, or - ultr_prs_loss_pw - this list's own entry of a [B, L] array (an estimator that reads the clicks).
//
// Numerics follow autograd through the reference's composition, quirks included:
//   x = 1 / (exp(-sigma s_ij) + 1) with the reciprocal-of-exp chain (no logistic shortcut), F.binary_cross_entropy with each
//   log clamped at -100, dL/dx = w (x - t) / max(x (1 - x), 1e-12), dx/dz = -x^2 * e.  x rounds to 1.0 for gaps above ~16.6 /
//   sigma, where the gradient explodes (1e-12 floor) instead of saturating; and where exp(sigma s_ij) overflows in the LOWER
//   triangle (gap above ~88.7 / sigma) its zero upstream gradient meets inf: both scores of the pair get NaN, as in torch.
// The batch-global IDCG is NOT applied: dscores and tail[0] are x D, tail[1] = this list's IDCG contribution (D), the update
// applies 1 / D - so the data-parallel exchange of the tail head carries the global IDCG with it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"

// expf(v) is +inf from here up (0x42B17218: the first float above ln(FLT_MAX))
#define PRS_EXP_OVERFLOW 88.72283935546875f

__global__ __launch_bounds__(LPW * LOSS_JW * 64) void prs_loss_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ labels,
                                                                    const float* __restrict__ ipw_table, int n_ipw,
                                                                    const float* __restrict__ ipw_bl, float sigma, int B, int L, float* __restrict__ dscores,
                                                                    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const PrsLds lay(L);
  const ListWave at = list_wave(L);
  const int lane = at.lane, lw = at.lw, jw = at.jw, b = at.b;
  float* sm_tail = smem + lay.tail;
  float* sm_d = smem + lay.d;
  float* sm_acc = smem + lay.acc;
  float* ms = smem + lay.s + lw * L;
  float* my = smem + lay.y + lw * L;
  float* ps = smem + lay.ps + lw * L;
  float* ls = smem + lay.ls + lw * L;
  float* gs = smem + lay.g + lw * L;
  float* ipws = smem + lay.ipw + lw * L;
  float* pws = smem + lay.pw + lw * L;
  int* pos = reinterpret_cast<int*>(smem + lay.pos) + lw * L;
  float* mt = sm_tail + lw * tail;
  for (int t = threadIdx.x; t < L; t += blockDim.x) sm_d[t] = 1.0f / log2f((float)t + 2.0f);
  stage_list(at, scores, labels, B, L, tail, mt, ms, my);
  __syncthreads();
  float idcg = 0.f;
  if (b < B && jw == 0) {
    for (int i = lane; i < L; i += 64) {
      const Ranked k = rank_by_counting(ms, my, L, i);
      // getPropensityForOneList(..., use_non_clicked_data=True): IPW_list[min(l, len - 1)] for every position (prs_rank.py:114)
      // ipw_bl: the estimator looked at this list's clicks (ultr_history_pw), a weight per entry [B, L]
      const float ipw = ipw_bl != nullptr ? ipw_bl[(int64_t)b * L + i] : ipw_table[i < n_ipw ? i : n_ipw - 1];
      pos[i] = k.rs;
      ps[k.rs] = k.s;
      ls[k.rs] = k.y;
      gs[k.rs] = k.gain;
      ipws[k.rs] = ipw;
      pws[k.rs] = (ipw == 0.f) ? 0.f : 1.0f / ipw;  // _safe_div (prs_rank.py:121)
      idcg += k.idcg;
    }
    idcg = wave_sum(idcg);
  }
  __syncthreads();  // the sorted arrays are visible to the list's other waves
  const int c0 = at.lo, c1 = at.hi;
  if (b < B) {
    for (int r = lane; r < L; r += 64) {
      const float sr = ps[r], lr_ = ls[r], gr = gs[r], dr = sm_d[r], ipwr = ipws[r], pwr = pws[r];
      float g = 0.f, li = 0.f;
      for (int c = c0; c < c1; ++c) {
        // the pair (i, j) = (min(r, c), max(r, c)) of the upper triangle; r == c gives x == t and no loss: contributes 0
        const bool up = c > r;
        const float sc = ps[c], lc = ls[c];
        const float s_ij = up ? sr - sc : sc - sr;
        const float y_ij = up ? lr_ - lc : lc - lr_;
        const float prs = up ? ipwr * pws[c] : ipws[c] * pwr;
        const float w = fabsf(gr - gs[c]) * fabsf(dr - sm_d[c]);     // delta-NDCG x IDCG (1/IDCG applied later)
        const float t = 0.5f * (1.0f + fminf(1.0f, fmaxf(y_ij, -1.0f)));
        const float a = -sigma * s_ij;
        const float e = expf(a);
        const float x = 1.0f / (e + 1.0f);
        // F.binary_cross_entropy element, each log clamped at -100, times the weight, times prs
        const float bce = (t - 1.0f) * fmaxf(log1pf(-x), -100.0f) - t * fmaxf(logf(x), -100.0f);
        li += up ? prs * (bce * w) : 0.f;
        // autograd: dL/dx = prs (x - t) / max((1 - x) x, 1e-12) w; reciprocal: * -x^2; exp: * e; * (-sigma)
        const float gx = prs * (x - t) / fmaxf((1.0f - x) * x, 1e-12f) * w;
        float gz = gx * -(x * x) * e * -sigma;
        if (-a >= PRS_EXP_OVERFLOW) gz = __builtin_nanf("");  // lower triangle: exp(-sigma s_ji) = inf meets a zero gradient
        g += up ? gz : -gz;
      }
      float* acc = slice_acc<2>(sm_acc, lw, jw, L, r);
      acc[0] = g;
      acc[1] = li;
    }
  }
  __syncthreads();
  if (b < B && jw == 0) {
    float lsum = 0.f;
    for (int r = lane; r < L; r += 64) {
      float v[2];
      fold_slices<2>(sm_acc, lw, L, r, v);
      ms[r] = v[0];  // raw scores are dead after the sort: reuse as d(loss)/d(sorted score r)
      lsum += v[1];
    }
    lsum = wave_sum(lsum);
    if (lane == 0) {
      mt[0] = lsum;
      mt[1] = idcg;
    }
  }
  scatter_sorted(at, B, L, ms, pos, dscores);
  store_wg_tail(sm_tail, tail, part + (int64_t)blockIdx.x * tail);
}

static int prs_launch(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, const float* ipw_bl,
                      float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  return launch_list_loss(prs_loss_kernel, LPW * LOSS_JW * 64, PrsLds(list_size).bytes, PrsLds::limit, batch, stream, scores, labels,
                          ipw_table, n_ipw, ipw_bl, sigma, batch, list_size, dscores, (float*)loss_ws);
}

extern "C" int ultr_prs_loss(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, float sigma,
                             int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  if (!scores || !labels || !ipw_table || n_ipw <= 0 || !dscores || !loss_ws || batch <= 0 || list_size <= 0)
    return ULTR_E_BADARG;
  return prs_launch(scores, labels, ipw_table, n_ipw, nullptr, sigma, batch, list_size, dscores, loss_ws, stream);
}

extern "C" int ultr_prs_loss_pw(const float* scores, const float* labels, const float* ipw_bl, float sigma, int32_t batch,
                                int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  if (!scores || !labels || !ipw_bl || !dscores || !loss_ws || batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  return prs_launch(scores, labels, nullptr, 0, ipw_bl, sigma, batch, list_size, dscores, loss_ws, stream);
}
