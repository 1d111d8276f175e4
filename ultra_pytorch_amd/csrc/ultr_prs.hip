// ultr_prs.hip — gfx950 loss kernel of PRSrank, the propensity-ratio-scored LambdaRank   (reference prs_rank.py:94-176, 207-251)
//
// The same decomposition as lambdarank_kernel (ultr_loss.hip): one list per workgroup, wave 0 of the list sorts by rank
// counting (ties broken by original index), then PRS_JW waves each walk a slice of the partner positions c for every sorted
// position r; the two partial sums per position (d loss / d sorted score, loss) are combined in fixed order through LDS.
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

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_prof.h"

#define LPW ULTR_LOSS_LISTS_PER_WG  // lists per workgroup
#ifndef PRS_JW
#define PRS_JW 16  // wavefronts per list (lambdarank_kernel's PD_JW)
#endif

// expf(v) is +inf from here up (0x42B17218: the first float above ln(FLT_MAX))
#define PRS_EXP_OVERFLOW 88.72283935546875f

__global__ __launch_bounds__(LPW * PRS_JW * 64) void prs_loss_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ labels,
                                                                    const float* __restrict__ ipw_table, int n_ipw,
                                                                    const float* __restrict__ ipw_bl, float sigma, int B, int L, float* __restrict__ dscores,
                                                                    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  float* sm_tail = smem;                // [LPW][tail]
  float* sm_s = sm_tail + LPW * tail;   // [LPW][L] raw scores, later d(loss)/d(sorted score)
  float* sm_y = sm_s + LPW * L;         // [LPW][L] raw labels
  float* sm_ps = sm_y + LPW * L;        // [LPW][L] scores sorted desc
  float* sm_ls = sm_ps + LPW * L;       // [LPW][L] labels in score order
  float* sm_g = sm_ls + LPW * L;        // [LPW][L] gains 2^l - 1 in score order
  float* sm_ipw = sm_g + LPW * L;       // [LPW][L] ipw of the presentation position, in score order
  float* sm_pw = sm_ipw + LPW * L;      // [LPW][L] pw = 1 / ipw (0 where ipw == 0), in score order
  float* sm_d = sm_pw + LPW * L;        // [L] discount 1 / log2(rank + 2)
  int* sm_pos = reinterpret_cast<int*>(sm_d + L);              // [LPW][L] sorted position of original index
  float* sm_acc = reinterpret_cast<float*>(sm_pos + LPW * L);  // [LPW][PRS_JW][L][2]: g, loss
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lw = wave / PRS_JW, jw = wave - lw * PRS_JW;
  const int b = blockIdx.x * LPW + lw;
  float* ms = sm_s + lw * L;
  float* my = sm_y + lw * L;
  float* ps = sm_ps + lw * L;
  float* ls = sm_ls + lw * L;
  float* gs = sm_g + lw * L;
  float* ipws = sm_ipw + lw * L;
  float* pws = sm_pw + lw * L;
  int* pos = sm_pos + lw * L;
  float* mt = sm_tail + lw * tail;
  for (int t = threadIdx.x; t < L; t += blockDim.x) sm_d[t] = 1.0f / log2f((float)t + 2.0f);
  if (jw == 0) {
    for (int t = lane; t < tail; t += 64) mt[t] = 0.f;
    if (b < B)
      for (int l = lane; l < L; l += 64) {
        ms[l] = scores[(int64_t)b * L + l];
        my[l] = labels[(int64_t)l * B + b];
      }
  }
  __syncthreads();
  float idcg = 0.f;
  if (b < B && jw == 0) {
    for (int i = lane; i < L; i += 64) {
      const float si = ms[i], yi = my[i];
      int rs = 0, ry = 0;
      for (int j = 0; j < L; ++j) {
        const float sj = ms[j], yj = my[j];
        rs += (sj > si || (sj == si && j < i)) ? 1 : 0;
        ry += (yj > yi || (yj == yi && j < i)) ? 1 : 0;
      }
      // getPropensityForOneList(..., use_non_clicked_data=True): IPW_list[min(l, len - 1)] for every position (prs_rank.py:114)
      // ipw_bl: the estimator looked at this list's clicks (ultr_history_pw), a weight per entry [B, L]
      const float ipw = ipw_bl != nullptr ? ipw_bl[(int64_t)b * L + i] : ipw_table[i < n_ipw ? i : n_ipw - 1];
      pos[i] = rs;
      ps[rs] = si;
      ls[rs] = yi;
      gs[rs] = exp2f(yi) - 1.0f;
      ipws[rs] = ipw;
      pws[rs] = (ipw == 0.f) ? 0.f : 1.0f / ipw;  // _safe_div (prs_rank.py:121)
      // dcg(): sum (2^l - 1) / ln(rank + 1), rank 1-based -> ln(ry + 2)   (prs_rank.py:207-226)
      idcg += (exp2f(yi) - 1.0f) / logf((float)ry + 2.0f);
    }
    idcg = wave_sum(idcg);
  }
  __syncthreads();  // the sorted arrays are visible to the list's other waves
  const int clen = (L + PRS_JW - 1) / PRS_JW, c0 = jw * clen, c1 = (c0 + clen < L) ? c0 + clen : L;
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
      float* acc = sm_acc + ((size_t)(lw * PRS_JW + jw) * L + r) * 2;
      acc[0] = g;
      acc[1] = li;
    }
  }
  __syncthreads();
  if (b < B && jw == 0) {
    float lsum = 0.f;
    for (int r = lane; r < L; r += 64) {
      float v0 = sm_acc[((size_t)(lw * PRS_JW) * L + r) * 2], v1 = sm_acc[((size_t)(lw * PRS_JW) * L + r) * 2 + 1];
#pragma unroll
      for (int w = 1; w < PRS_JW; ++w) {
        v0 += sm_acc[((size_t)(lw * PRS_JW + w) * L + r) * 2];
        v1 += sm_acc[((size_t)(lw * PRS_JW + w) * L + r) * 2 + 1];
      }
      ms[r] = v0;  // raw scores are dead after the sort: reuse as d(loss)/d(sorted score r)
      lsum += v1;
    }
    lsum = wave_sum(lsum);
    if (lane == 0) {
      mt[0] = lsum;
      mt[1] = idcg;
    }
  }
  // ms[] (now gradients by sorted position) written by lane r, read by the lane owning the original index
  __syncthreads();
  if (b < B && jw == 0)
    for (int i = lane; i < L; i += 64) dscores[(int64_t)b * L + i] = ms[pos[i]];
  // the workgroup's partial: its lists' tails summed in fixed order
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * tail;
  for (int t = threadIdx.x; t < tail; t += blockDim.x) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LPW; ++w) s += sm_tail[w * tail + t];
    out[t] = s;
  }
}

static size_t prs_lds_bytes(int32_t list_size) {
  const int tail = (int)ultr_tail_len(list_size);
  return ((size_t)LPW * (tail + 8 * (size_t)list_size) + list_size + (size_t)LPW * PRS_JW * list_size * 2) * sizeof(float);
}

static int prs_launch(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, const float* ipw_bl,
                      float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  const size_t lds = prs_lds_bytes(list_size);
  if (lds > 160 * 1024) return ULTR_E_UNSUPPORTED;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(prs_loss_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  UltrProfScope prof(ULTR_K_LOSS, (hipStream_t)stream);
  ULTR_LAUNCH(prof, prs_loss_kernel, dim3((unsigned)ultr_loss_parts(batch)), dim3(LPW * PRS_JW * 64), lds, (hipStream_t)stream,
              scores, labels, ipw_table, (int)n_ipw, ipw_bl, sigma, (int)batch, (int)list_size, dscores, (float*)loss_ws);
  return (int)hipGetLastError();
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
