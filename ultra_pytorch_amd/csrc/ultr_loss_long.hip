// ultr_loss_long.hip — the pair-walk list losses (PairDebias, LambdaRank, PRSrank) for lists the short kernels refuse
//
// pairdebias_kernel, lambdarank_kernel (ultr_loss.hip) and prs_loss_kernel (ultr_prs.hip) let the LOSS_JW waves of a list split the
// PARTNER range, so every position's partial sums are folded through a [LOSS_JW][L][NV] array in LDS: that array bounds them at 585 /
// 531 / 952 documents.  The kernels here split the OWNED positions over the workgroup's 16 waves instead: thread t owns the positions
// t, t + 1024, ... and walks ALL partners 0 .. L-1 in ascending order, so its sums live in registers and go straight to dscores and
// the tail.  What stays in LDS is O(L) (PairDebiasLongLds, LambdaRankLongLds, PrsLongLds in ultr_listloss.h): 6823 / 3149 / 3721
// documents at 160 KiB.  Every lane of a wave reads the same partner: the LDS reads of the walk are broadcasts.
//
// The per-pair expressions are the short kernels', restated (the short kernels' code, and so their bits, stay as they are); a
// position's sum is an ascending fold of the sums of LOSS_LONG_CHUNK consecutive partners (a chain of 1251 fp32 additions rounds
// several times worse) where the short kernels fold LOSS_JW slice sums, so the two agree to rounding, not bit for bit.  The rank-by-counting sort (L^2 compares) is spread over all 16 waves, same stable order.  One
// workgroup per list, one tail partial per workgroup, the tail contract of ultr_loss.hip unchanged; workgroup-wide sums (loss, ideal
// DCG) go wave by wave through LDS in fixed order.  No atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_listloss.h"

#define PRS_EXP_OVERFLOW 88.72283935546875f  // expf(v) is +inf from here up (ultr_prs.hip)

// the workgroup's sum of v in fixed order: lanes by wave_sum, then the waves 0, 1, ..., LOSS_LONG_WAVES - 1; every thread calls it
__device__ __forceinline__ float wg_sum(float v, float* red /*[LOSS_LONG_WAVES]*/) {
  v = wave_sum(v);
  __syncthreads();  // (an earlier sum's readers are done with red)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < LOSS_LONG_WAVES; ++w) s += red[w];
  return s;
}

// the whole workgroup zeroes the list's tail and stages its raw scores [B, L] and labels [L, B]
__device__ __forceinline__ void stage_list_long(const float* __restrict__ scores, const float* __restrict__ labels, int b, int B, int L,
                                                int tail, float* mt, float* ms, float* my) {
  for (int t = threadIdx.x; t < tail; t += LOSS_LONG_THREADS) mt[t] = 0.f;
  for (int l = threadIdx.x; l < L; l += LOSS_LONG_THREADS) {
    ms[l] = scores[(int64_t)b * L + l];
    my[l] = labels[(int64_t)l * B + b];
  }
}

// ------------------------------------------------------------------------------------------------
// PairDebias                                                    pairwise_debias.py:142-157
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_LONG_THREADS) void pairdebias_long_kernel(const float* __restrict__ scores,
                                                                            const float* __restrict__ labels,
                                                                            const float* __restrict__ t_plus,
                                                                            const float* __restrict__ t_minus, int B, int L, float bscale,
                                                                            float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const PairDebiasLongLds lay(L);
  const int b = blockIdx.x;  // one list per workgroup, the grid is the batch
  float* mt = smem + lay.tail;
  float* ms = smem + lay.s;
  float* mc = smem + lay.c;
  float* sm_rtp = smem + lay.rtp;
  float* sm_rtm = smem + lay.rtm;
  float* red = smem + lay.red;
  for (int t = threadIdx.x; t < L; t += LOSS_LONG_THREADS) {
    sm_rtp[t] = 1.0f / t_plus[t];
    sm_rtm[t] = 1.0f / t_minus[t];
  }
  stage_list_long(scores, labels, b, B, L, tail, mt, ms, mc);
  __syncthreads();
  float lsum = 0.f;
  for (int i = threadIdx.x; i < L; i += LOSS_LONG_THREADS) {
    const float si = ms[i], ci = mc[i], rtpi = sm_rtp[i], rtmi = sm_rtm[i];
    float g = 0.f, tpl = 0.f, tml = 0.f, li = 0.f;
    for (int j0 = 0; j0 < L; j0 += LOSS_LONG_CHUNK) {
      const int j1 = (j0 + LOSS_LONG_CHUNK < L) ? j0 + LOSS_LONG_CHUNK : L;
      float cg = 0.f, ctpl = 0.f, ctml = 0.f, cli = 0.f;
      for (int j = j0; j < j1; ++j) {
        const float dc = ci - mc[j];                 // > 0: (i, j) is the valid pair; < 0: (j, i); 0 (incl. j == i): neither
        const bool fwd = dc > 0.f;
        const float m = fminf(1.0f, fabsf(dc));      // valid_pair_mask value
        const float x = fwd ? ms[j] - si : si - ms[j];   // s_neg - s_pos of the valid ordered pair
        const float e = __expf(-fabsf(x));
        const float r = 1.0f / (1.0f + e);
        const float sp = fmaxf(x, 0.f) + log1pf(e);      // softplus(x)
        const float sg = (x >= 0.f) ? r : e * r;         // sigmoid(x)
        const float pl = bscale * m * sp;                // PL contribution of this list (x B)
        const float gw = bscale * m * sg;
        const float rj = fwd ? sm_rtm[j] : sm_rtp[j];    // 1 / t_minus[j]  or  1 / t_plus[j]
        // (i, j): t_plus_loss[i] += PL_ij / t-_j; loss += PL_ij / t+_i / t-_j; d/ds_i = -gw / t+_i / t-_j
        // (j, i): t_minus_loss[i] += PL_ji / t+_j;                              d/ds_i = +gw / t+_j / t-_i
        const float plr = pl * rj;
        ctpl += fwd ? plr : 0.f;
        ctml += fwd ? 0.f : plr;
        cli += fwd ? plr * rtpi : 0.f;
        cg += fwd ? -(gw * rj * rtpi) : gw * rj * rtmi;
      }
      g += cg, tpl += ctpl, tml += ctml, li += cli;
    }
    dscores[(int64_t)b * L + i] = g;
    mt[ULTR_TAIL_FIXED + i] = tpl;
    mt[ULTR_TAIL_FIXED + L + i] = tml;
    lsum += li;
  }
  lsum = wg_sum(lsum, red);
  if (threadIdx.x == 0) {
    mt[0] = lsum;
    mt[1] = 1.0f;  // unused normaliser
  }
  store_wg_tail(mt, tail, part + (int64_t)blockIdx.x * tail);
}

// ------------------------------------------------------------------------------------------------
// the sort of the two sorted kernels: thread t ranks the positions t, t + 1024, ... (stable, ties by original index) and moves
// them to score order; `own(i, rank)` moves what else the kernel keeps per position.  Returns the list's ideal DCG.
// ------------------------------------------------------------------------------------------------
template <class Own>
__device__ __forceinline__ float sort_list_long(const float* ms, const float* my, int L, float* ps, float* ls, float* gs, int* pos,
                                                float* red, Own own) {
  float idcg = 0.f;
  for (int i = threadIdx.x; i < L; i += LOSS_LONG_THREADS) {
    const Ranked k = rank_by_counting(ms, my, L, i);
    pos[i] = k.rs;
    ps[k.rs] = k.s;
    ls[k.rs] = k.y;
    gs[k.rs] = k.gain;
    own(i, k.rs);
    idcg += k.idcg;
  }
  return wg_sum(idcg, red);  // (its barriers also make the sorted arrays visible to every wave)
}

// gradients by sorted position (ms[], written by the thread of the sorted position) to presentation order
__device__ __forceinline__ void scatter_sorted_long(int b, int L, const float* ms, const int* pos, float* __restrict__ dscores) {
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += LOSS_LONG_THREADS) dscores[(int64_t)b * L + i] = ms[pos[i]];
}

// ------------------------------------------------------------------------------------------------
// LambdaRank                                                    lambda_rank.py:116-135, 247-291
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_LONG_THREADS) void lambdarank_long_kernel(const float* __restrict__ scores,
                                                                            const float* __restrict__ labels,
                                                                            const float* __restrict__ t_plus,
                                                                            const float* __restrict__ t_minus, float sigma, int B, int L,
                                                                            float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const LambdaRankLongLds lay(L);
  const int b = blockIdx.x;
  float* mt = smem + lay.tail;
  float* sm_tp = smem + lay.tp;
  float* sm_tm = smem + lay.tm;
  float* sm_rtp = smem + lay.rtp;
  float* sm_rtm = smem + lay.rtm;
  float* sm_d = smem + lay.d;
  float* ms = smem + lay.s;
  float* my = smem + lay.y;
  float* ps = smem + lay.ps;
  float* ls = smem + lay.ls;
  float* gs = smem + lay.g;
  int* pos = reinterpret_cast<int*>(smem + lay.pos);
  float* red = smem + lay.red;
  for (int t = threadIdx.x; t < L; t += LOSS_LONG_THREADS) {
    const float tp = t_plus[t], tm = t_minus[t];
    sm_tp[t] = tp;
    sm_tm[t] = tm;
    sm_rtp[t] = 1.0f / tp;
    sm_rtm[t] = 1.0f / tm;
    sm_d[t] = 1.0f / log2f((float)t + 2.0f);
  }
  stage_list_long(scores, labels, b, B, L, tail, mt, ms, my);
  __syncthreads();
  const float idcg = sort_list_long(ms, my, L, ps, ls, gs, pos, red, [](int, int) {});
  float lsum = 0.f;
  for (int r = threadIdx.x; r < L; r += LOSS_LONG_THREADS) {
    const float sr = ps[r], lr_ = ls[r], gr = gs[r], tpr = sm_tp[r], tmr = sm_tm[r], rtpr = sm_rtp[r], rtmr = sm_rtm[r];
    const float dr = sm_d[r];
    float g = 0.f, tpl = 0.f, tml = 0.f, li = 0.f;
    for (int c0 = 0; c0 < L; c0 += LOSS_LONG_CHUNK) {
      const int c1 = (c0 + LOSS_LONG_CHUNK < L) ? c0 + LOSS_LONG_CHUNK : L;
      float cg = 0.f, ctpl = 0.f, ctml = 0.f, cli = 0.f;
      for (int c = c0; c < c1; ++c) {
        const float delta = fabsf(gr - gs[c]) * fabsf(dr - sm_d[c]);        // x 1/IDCG applied later
        const float S = fminf(1.0f, fmaxf(lr_ - ls[c], -1.0f));
        const float pb_rc = 0.5f * (1.0f + S), pb_cr = 0.5f * (1.0f - S);
        const float z = sigma * (sr - ps[c]);
        const float ez = __expf(-fabsf(z));
        const float r0 = 1.0f / (1.0f + ez);
        const float xhi = r0, xlo = ez * r0;                                // sigmoid(|z|), sigmoid(-|z|)
        const float x_rc = (z >= 0.f) ? xhi : xlo, x_cr = (z >= 0.f) ? xlo : xhi;
        // BCEWithLogits on a probability x in (0, 1): x - x t + log1p(exp(-x)); derivative sigmoid(x) - t
        const float e1 = __expf(-x_rc), e2 = __expf(-x_cr);
        const float l_rc = delta * (x_rc - x_rc * pb_rc + log1pf(e1));      // PL[r, c] contribution
        const float l_cr = delta * (x_cr - x_cr * pb_cr + log1pf(e2));      // PL[c, r]
        const float rtmc = sm_rtm[c], rtpc = sm_rtp[c];
        const bool ok_rc = (tpr * sm_tm[c]) != 0.f, ok_cr = (sm_tp[c] * tmr) != 0.f;   // _safe_div
        ctpl += l_rc * rtmc;   // t_plus_loss[r]  = sum_c PL[r,c] / t_minus[c]
        ctml += l_cr * rtpc;   // t_minus_loss[r] = sum_c PL[c,r] / t_plus[c]
        cli += ok_rc ? l_rc * rtpr * rtmc : 0.f;
        // d PL[r,c]/d s_r  and  d PL[c,r]/d s_r  (x = sigmoid(+-z): dx/ds_r = +-sigma x (1 - x), x (1 - x) = xhi xlo)
        const float xx = sigma * xhi * xlo;
        const float d_rc = delta * (1.0f / (1.0f + e1) - pb_rc) * xx;
        const float d_cr = delta * (1.0f / (1.0f + e2) - pb_cr) * xx;
        cg += ok_rc ? d_rc * rtpr * rtmc : 0.f;
        cg -= ok_cr ? d_cr * rtpc * rtmr : 0.f;
      }
      g += cg, tpl += ctpl, tml += ctml, li += cli;
    }
    mt[ULTR_TAIL_FIXED + r] = tpl;
    mt[ULTR_TAIL_FIXED + L + r] = tml;
    ms[r] = g;  // raw scores are dead after the sort: reuse as d(loss)/d(sorted score r)
    lsum += li;
  }
  lsum = wg_sum(lsum, red);
  if (threadIdx.x == 0) {
    mt[0] = lsum;
    mt[1] = idcg;
  }
  scatter_sorted_long(b, L, ms, pos, dscores);
  store_wg_tail(mt, tail, part + (int64_t)blockIdx.x * tail);
}

// ------------------------------------------------------------------------------------------------
// PRSrank                                                       prs_rank.py:94-176, 207-251
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_LONG_THREADS) void prs_loss_long_kernel(const float* __restrict__ scores,
                                                                          const float* __restrict__ labels,
                                                                          const float* __restrict__ ipw_table, int n_ipw,
                                                                          const float* __restrict__ ipw_bl, float sigma, int B, int L,
                                                                          float* __restrict__ dscores, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tail = (int)ultr_tail_len(L);
  const PrsLongLds lay(L);
  const int b = blockIdx.x;
  float* mt = smem + lay.tail;
  float* sm_d = smem + lay.d;
  float* ms = smem + lay.s;
  float* my = smem + lay.y;
  float* ps = smem + lay.ps;
  float* ls = smem + lay.ls;
  float* gs = smem + lay.g;
  float* ipws = smem + lay.ipw;
  float* pws = smem + lay.pw;
  int* pos = reinterpret_cast<int*>(smem + lay.pos);
  float* red = smem + lay.red;
  for (int t = threadIdx.x; t < L; t += LOSS_LONG_THREADS) sm_d[t] = 1.0f / log2f((float)t + 2.0f);
  stage_list_long(scores, labels, b, B, L, tail, mt, ms, my);
  __syncthreads();
  const float idcg = sort_list_long(ms, my, L, ps, ls, gs, pos, red, [&](int i, int rs) {
    // getPropensityForOneList(..., use_non_clicked_data=True): IPW_list[min(l, len - 1)] for every position (prs_rank.py:114)
    // ipw_bl: the estimator looked at this list's clicks (ultr_history_pw), a weight per entry [B, L]
    const float ipw = ipw_bl != nullptr ? ipw_bl[(int64_t)b * L + i] : ipw_table[i < n_ipw ? i : n_ipw - 1];
    ipws[rs] = ipw;
    pws[rs] = (ipw == 0.f) ? 0.f : 1.0f / ipw;  // _safe_div (prs_rank.py:121)
  });
  float lsum = 0.f;
  for (int r = threadIdx.x; r < L; r += LOSS_LONG_THREADS) {
    const float sr = ps[r], lr_ = ls[r], gr = gs[r], dr = sm_d[r], ipwr = ipws[r], pwr = pws[r];
    float g = 0.f, li = 0.f;
    for (int c0 = 0; c0 < L; c0 += LOSS_LONG_CHUNK) {
      const int c1 = (c0 + LOSS_LONG_CHUNK < L) ? c0 + LOSS_LONG_CHUNK : L;
      float cg = 0.f, cli = 0.f;
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
        cli += up ? prs * (bce * w) : 0.f;
        // autograd: dL/dx = prs (x - t) / max((1 - x) x, 1e-12) w; reciprocal: * -x^2; exp: * e; * (-sigma)
        const float gx = prs * (x - t) / fmaxf((1.0f - x) * x, 1e-12f) * w;
        float gz = gx * -(x * x) * e * -sigma;
        if (-a >= PRS_EXP_OVERFLOW) gz = __builtin_nanf("");  // lower triangle: exp(-sigma s_ji) = inf meets a zero gradient
        cg += up ? gz : -gz;
      }
      g += cg, li += cli;
    }
    ms[r] = g;  // raw scores are dead after the sort: reuse as d(loss)/d(sorted score r)
    lsum += li;
  }
  lsum = wg_sum(lsum, red);
  if (threadIdx.x == 0) {
    mt[0] = lsum;
    mt[1] = idcg;
  }
  scatter_sorted_long(b, L, ms, pos, dscores);
  store_wg_tail(mt, tail, part + (int64_t)blockIdx.x * tail);
}

// ------------------------------------------------------------------------------------------------
// entries: the arguments and the ULTR_E_BADARG rules of the short ones; every list_size from 1 up to the layout's bound
// ------------------------------------------------------------------------------------------------
extern "C" int64_t ultr_loss_long_lds_bytes(int32_t algo, int32_t list_size) { return loss_long_bytes(algo, list_size); }

extern "C" int32_t ultr_loss_long_max_list(int32_t algo) {
  if (loss_long_bytes(algo, 1) < 0) return ULTR_E_BADARG;
  int lo = 1, hi = INT32_MAX;  // the layouts grow with L: the last length whose bytes fit
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (loss_long_bytes(algo, mid) >= 0) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

extern "C" int ultr_pairdebias_loss_long(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                                         int32_t batch, int32_t list_size, int32_t batch_total, float* dscores, void* loss_ws,
                                         void* stream) {
  if (!scores || !labels || !t_plus || !t_minus || !dscores || !loss_ws || batch <= 0 || list_size <= 0 || batch_total <= 0)
    return ULTR_E_BADARG;
  return launch_list_loss(pairdebias_long_kernel, LOSS_LONG_THREADS, PairDebiasLongLds(list_size).bytes, PairDebiasLongLds::limit, batch,
                          stream, scores, labels, t_plus, t_minus, batch, list_size, batch_total, dscores, (float*)loss_ws);
}

extern "C" int ultr_lambdarank_loss_long(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                                         float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  if (!scores || !labels || !t_plus || !t_minus || !dscores || !loss_ws || batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  return launch_list_loss(lambdarank_long_kernel, LOSS_LONG_THREADS, LambdaRankLongLds(list_size).bytes, LambdaRankLongLds::limit, batch,
                          stream, scores, labels, t_plus, t_minus, sigma, batch, list_size, dscores, (float*)loss_ws);
}

static int prs_long_launch(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, const float* ipw_bl,
                           float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  return launch_list_loss(prs_loss_long_kernel, LOSS_LONG_THREADS, PrsLongLds(list_size).bytes, PrsLongLds::limit, batch, stream, scores,
                          labels, ipw_table, n_ipw, ipw_bl, sigma, batch, list_size, dscores, (float*)loss_ws);
}

extern "C" int ultr_prs_loss_long(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, float sigma,
                                  int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  if (!scores || !labels || !ipw_table || n_ipw <= 0 || !dscores || !loss_ws || batch <= 0 || list_size <= 0)
    return ULTR_E_BADARG;
  return prs_long_launch(scores, labels, ipw_table, n_ipw, nullptr, sigma, batch, list_size, dscores, loss_ws, stream);
}

extern "C" int ultr_prs_loss_pw_long(const float* scores, const float* labels, const float* ipw_bl, float sigma, int32_t batch,
                                     int32_t list_size, float* dscores, void* loss_ws, void* stream) {
  if (!scores || !labels || !ipw_bl || !dscores || !loss_ws || batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  return prs_long_launch(scores, labels, nullptr, 0, ipw_bl, sigma, batch, list_size, dscores, loss_ws, stream);
}
