// ultr_update.hip — clip + optimizer + EM / propensity updates, one launch per step.
//
// Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.Adagrad.step / SGD.step (reference
// base_algorithm.py:208-226), DLA.separate_gradient_update (dla.py:141-177) and the t_plus / t_minus EM
// updates (pairwise_debias.py:159-163, lambda_rank.py:136-142).  Every workgroup recomputes the handful of
// step scalars (global normaliser, gradient norm, clip coefficient) from the same inputs in the same order,
// so no grid barrier and no atomics are needed and all workgroups agree bit-for-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_feed.h"
#include "ultr_prof.h"

// Optional phase tracing (-DULTR_TRACE, as ultr_dnn_kernels.h): update_tiled_kernel stamps bank 2 of this unit's array - 0 entry,
// 1 indices known, 2 gradient / parameter / state words arrived, 3 after the sum-of-squares block sum, 4 end (tools/trace_phases.py)
#ifdef ULTR_TRACE
static __device__ unsigned long long g_upd_trace[3 * 64 * 32];
#define UPD_STAMP(slot)                                                                        \
  do {                                                                                         \
    if (threadIdx.x == 0 && (blockIdx.x & 31) == 0 && (blockIdx.x >> 5) < 64)                  \
      g_upd_trace[2 * 2048 + (blockIdx.x >> 5) * 32 + (slot)] = __builtin_amdgcn_s_memtime();  \
  } while (0)
#define UPD_AFTER(v) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(v) : "memory")
int ultr_trace_read_update(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_upd_trace), sizeof(unsigned long long) * 3 * 64 * 32);
}
#else
#define UPD_STAMP(slot) \
  do {                  \
  } while (0)
#define UPD_AFTER(v) \
  do {               \
  } while (0)
#endif

__device__ __forceinline__ float block_sum256(float v, float* sm) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__device__ __forceinline__ float opt_step(float p, float g, float* st, int opt, bool stateless, float lr, float eps) {
  if (opt == ULTR_OPT_SGD) return p - lr * g;
  // torch.optim.Adagrad (lr_decay 0, weight_decay 0, initial accumulator 0): s += g*g; p -= lr * g / (sqrt(s) + eps).
  // stateless: DLA builds fresh optimizers every step (dla.py:153-154) -> the accumulator is always g*g.
  const float s = (stateless ? 0.f : *st) + g * g;
  if (!stateless) *st = s;
  return p - lr * (g / (sqrtf(s) + eps));
}

// ULTR_OPT_ADAM.  The bias corrections depend on the step count alone, so the HOST forms them, in double (adam_corr): a float32
// pow(b2, t) in every thread would cost more than the rest of the step and lose digits as t grows.
//   step  = lr / (1 - b1^t)   (step_aux: the same with propensity_learning_rate, for DLA's aux and TwoTower's)
//   rsq2  = 1 / sqrt(1 - b2^t)
// The kernels are instantiated per optimizer class; the Adagrad / SGD instantiation carries an empty OptArgs.
template <bool ADAM>
struct OptArgs {};
template <>
struct OptArgs<true> {
  float step, step_aux, rsq2;
};
static OptArgs<true> adam_corr(const ultr_update_desc& u) {
  const double t = (double)u.adam_t;
  const double bc1 = 1.0 - pow(ULTR_ADAM_BETA1, t), bc2 = 1.0 - pow(ULTR_ADAM_BETA2, t);
  OptArgs<true> oa;
  oa.step = (float)((double)u.learning_rate / bc1);
  oa.step_aux = (float)((double)u.propensity_learning_rate / bc1);
  oa.rsq2 = (float)(1.0 / sqrt(bc2));
  return oa;
}
// torch.optim.Adam (weight_decay 0, amsgrad off): m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
// p -= step * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  g == 0 on fresh moments: m / eps = 0, p stays.
__device__ __forceinline__ float adam_step(float p, float g, float* m, float* v, float step, float rsq2, float eps) {
  const float b1 = (float)ULTR_ADAM_BETA1, b2 = (float)ULTR_ADAM_BETA2;
  const float mn = b1 * *m + (float)(1.0 - ULTR_ADAM_BETA1) * g;
  const float vn = b2 * *v + (float)(1.0 - ULTR_ADAM_BETA2) * (g * g);
  *m = mn;
  *v = vn;
  return p - step * (mn / (sqrtf(vn) * rsq2 + eps));
}

// Step report into HOST-mapped pinned memory (ultr_update_desc::host_scalars): eight scalars + the guard word, waited for
// (the stores are acknowledged by the host bridge), THEN the sequence number the host spins on - what loss.item() costs
// becomes one posted PCIe write instead of a stream synchronisation and a device-to-host copy.
__device__ __forceinline__ void host_report(const ultr_update_desc& u, const float (&v)[8], uint32_t status) {
  float* hs = u.host_scalars;
#pragma unroll
  for (int k = 0; k < 8; ++k) __hip_atomic_store(hs + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(reinterpret_cast<uint32_t*>(hs) + 8, status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(reinterpret_cast<uint32_t*>(hs) + 9, u.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // [10]: "the loss of step seq is in [0]" - already raised by the weight-gradient launch when an early report was possible
  __hip_atomic_store(reinterpret_cast<uint32_t*>(hs) + 10, u.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// This thread's share of the sum of the level-1 sum-of-squares partials, ASSOCIATED AS THE LEVEL-2 PATH WOULD: groups of four in
// order, ((p[4j] + p[4j+1]) + p[4j+2]) + p[4j+3] with missing partials = 0 (exactly what the reduction launches store as level-2
// partial j), thread t taking groups t, t + 256, ...  A data-parallel step may reach the update through the exchange inside the slab
// reduction (level-2 partials) on one rank and through the stand-alone exchange (level-1 only) on another - unequal local batches -
// and both must produce the SAME bits for the gradient norm and the clip coefficient, or the replicas fork.
__device__ __forceinline__ float sumsq_level1_as_level2(const float* __restrict__ part, int nsq, int t) {
  float ss = 0.f;
  const int ngroups = (nsq + 3) >> 2;
  for (int j = t; j < ngroups; j += 256) {
    const int k = 4 * j;
    const float p0 = part[k], p1 = k + 1 < nsq ? part[k + 1] : 0.f, p2 = k + 2 < nsq ? part[k + 2] : 0.f, p3 = k + 3 < nsq ? part[k + 3] : 0.f;
    ss += ((p0 + p1) + p2) + p3;
  }
  return ss;
}

// guard word set (a timed-out gradient exchange on this rank or on a peer): the launch must change nothing.  Block 0 still
// reports, with the status, so that the host's read of the loss raises instead of waiting for a sequence number forever.
__device__ __forceinline__ bool update_guarded(const ultr_update_desc& u) {
  if (u.guard == nullptr) return false;
  const uint32_t gv = __hip_atomic_load(u.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (gv == 0u) return false;
  if (blockIdx.x == 0 && threadIdx.x == 0 && u.host_scalars != nullptr) {
    const float nanv = __uint_as_float(0x7fc00000u);
    const float v[8] = {nanv, nanv, 0.f, 0.f, nanv, nanv, 0.f, 0.f};
    host_report(u, v, gv);
  }
  return true;
}

// pre-pass of ultr_apply_update when l2_loss > 0: out[0] = sum p^2, out[1] = sum g.p over the P parameters (one workgroup,
// fixed order: thread-strided partials, wave sums, 16 wave partials added in order)
__global__ __launch_bounds__(1024) void l2_sums_kernel(const float* __restrict__ params, const float* __restrict__ grads,
                                                       int64_t P, float* __restrict__ out) {
  __shared__ float sm[2][16];
  float a = 0.f, b = 0.f;
  for (int64_t e = threadIdx.x; e < P; e += 1024) {
    const float p = params[e];
    a += p * p;
    b += grads[e] * p;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sm[0][threadIdx.x >> 6] = a;
    sm[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sa = 0.f, sb = 0.f;
    for (int w = 0; w < 16; ++w) {
      sa += sm[0][w];
      sb += sm[1][w];
    }
    out[0] = sa;
    out[1] = sb;
  }
}

// Everything after the gradient and the sum of squares are known: step scalars, clip, optimizer, k-major copy /
// image, and (block 0) the per-position state.  EPT elements per thread, indices e_a (-1 = none); the new parameter
// values come back in p_new_a for the caller's k-major / image writes.
// ADAM: s_old_a holds the first moments m = state[e] and v_old_a the second moments v = state[P + e]; DLA's aux moments and TwoTower's
// follow at state[2 P] (ultr_opt_state_floats).  Otherwise v_old_a is not read.
template <int EPT, bool ADAM>
__device__ __forceinline__ void update_body(const ultr_update_desc& u, const DnnPlan& dp, float* __restrict__ params,
                                            float* __restrict__ state, const float* __restrict__ tail,
                                            float* __restrict__ aux, float ss, const int64_t (&e_a)[EPT],
                                            const float (&g_raw_a)[EPT], const float (&p_old_a)[EPT],
                                            const float (&s_old_a)[EPT], const float (&v_old_a)[EPT], const OptArgs<ADAM>& oa,
                                            float (&p_new_a)[EPT], float* sm,
                                            float* __restrict__ scalars_out, const float* __restrict__ l2_sums,
                                            const uint32_t* __restrict__ h3flag = nullptr) {
  const int64_t P = u.n_params;
  const int L = u.list_size;
  const float loss_sum = tail[0], D = (u.algo == ULTR_ALGO_PDGD || u.algo == ULTR_ALGO_DBGD) ? 1.0f : tail[1], loss2 = tail[2], D2 = tail[3];
  float gs = 1.0f, loss = loss_sum, rank_loss = 0.f, exam_loss = 0.f;
  switch (u.algo) {
    case ULTR_ALGO_SOFTMAX:  // loss = sum_b loss_b / sum w   (base_algorithm.py:330)
      gs = 1.0f / D;
      loss = loss_sum / D;
      break;
    case ULTR_ALGO_DLA:  // loss = exam_loss + ranker_loss_weight * rank_loss   (dla.py:237)
      rank_loss = loss_sum / D;
      exam_loss = loss2 / D2;
      gs = u.ranker_loss_weight / D;
      loss = exam_loss + u.ranker_loss_weight * rank_loss;
      break;
    case ULTR_ALGO_PAIRDEBIAS:
      gs = 1.0f;
      loss = loss_sum;
      break;
    case ULTR_ALGO_LAMBDARANK:  // gains are normalised by the batch-global IDCG (lambda_rank.py:280-282)
      gs = 1.0f / D;
      loss = loss_sum / D;
      break;
    case ULTR_ALGO_REGEM:  // BCEWithLogits, mean over the D = B*L elements (regression_EM.py:149-151)
      gs = 1.0f / D;
      loss = loss_sum / D;
      break;
    case ULTR_ALGO_PRS:  // delta-NDCG weights are normalised by the batch-global IDCG (prs_rank.py:240)
      gs = 1.0f / D;
      loss = loss_sum / D;
      break;
    case ULTR_ALGO_TWOTOWER:  // the click log-likelihood: positions summed, mean over the D lists (ultr_twotower.hip)
    case ULTR_ALGO_PLRANK:    // minus the sampled expected DCG@K, mean over the D lists (ultr_plrank.hip)
    case ULTR_ALGO_AFFINE:    // the affine-corrected softmax loss, mean over the D lists; it may be negative (ultr_affine.hip)
      gs = 1.0f / D;
      loss = loss_sum / D;
      break;
    case ULTR_ALGO_PDGD:  // the weighted pair terms are summed (pdgd.py:197-205)
    case ULTR_ALGO_DBGD:  // grads already hold the step's direction; the loss is 1 - NDCG of the current model (dbgd.py:140)
      gs = 1.0f;
      loss = loss_sum;
      break;
  }
  float norm = fabsf(gs) * sqrtf(ss);
  // l2_loss > 0 (ipw_rank.py:154-157 and siblings): g += lam * p, loss += l2_loss * sum p^2 / 2.  Every algorithm but DLA
  // and PDGD hands clip_grad_norm_ a parameter generator the L2 loop has already exhausted, so NOTHING is clipped (Appendix
  // A.8); DLA adds the term to rank_loss (scaled by ranker_loss_weight with it) and clips the full gradient (dla.py:146-162);
  // PDGD passes a FRESH model.parameters() to opt_step (pdgd.py:206-212) and clips the full gradient too.  TwoTower, PLRank and
  // AffineRank are the project's own algorithms and do not inherit the quirk: their clip covers the full gradient.
  float lam = 0.f;
  bool clip = u.max_gradient_norm > 0.f;
  if (u.l2_loss > 0.f && l2_sums != nullptr) {
    const float sp2 = l2_sums[0], sgp = l2_sums[1];
    if (u.algo == ULTR_ALGO_DLA) {
      lam = u.ranker_loss_weight * u.l2_loss;
      rank_loss += u.l2_loss * (0.5f * sp2);
      loss = exam_loss + u.ranker_loss_weight * rank_loss;
    } else {
      lam = u.l2_loss;
      loss += u.l2_loss * (0.5f * sp2);
      clip = clip && (u.algo == ULTR_ALGO_PDGD || u.algo == ULTR_ALGO_TWOTOWER || u.algo == ULTR_ALGO_PLRANK ||
                      u.algo == ULTR_ALGO_AFFINE);
    }
    norm = sqrtf(fmaxf(gs * gs * ss + 2.0f * gs * lam * sgp + lam * lam * sp2, 0.f));
  }
  const float coef = clip ? fminf(1.0f, u.max_gradient_norm / (norm + 1e-6f)) : 1.0f;
  const bool stateless = (u.algo == ULTR_ALGO_DLA);
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int64_t e = e_a[k];  // -1: no element
    const float g_raw = g_raw_a[k], p_old = p_old_a[k], s_old = s_old_a[k];
    p_new_a[k] = 0.f;
    if (e >= 0 && e < P) {
      float g = g_raw * gs;
      if (lam != 0.f) g += lam * p_old;
      g *= coef;
      if constexpr (ADAM) {
        float m_new = s_old, v_new = v_old_a[k];
        const float pn = adam_step(p_old, g, &m_new, &v_new, oa.step, oa.rsq2, u.adagrad_eps);
        params[e] = pn;
        state[e] = m_new;
        state[P + e] = v_new;
        p_new_a[k] = pn;
      } else {
        float s_new = s_old;
        const float pn = opt_step(p_old, g, &s_new, u.optimizer, stateless || state == nullptr, u.learning_rate, u.adagrad_eps);
        params[e] = pn;
        if (state != nullptr && !stateless && u.optimizer != ULTR_OPT_SGD) state[e] = s_new;
        p_new_a[k] = pn;
      }
    }
  }
  if (blockIdx.x != 0) return;
  // ---- block 0: step scalars + the small per-position state -----------------------------------------
  float pnorm = 0.f;
  if (u.algo == ULTR_ALGO_DLA && aux != nullptr) {
    // DenoisingNet backward: propensity[b,l] = ELU(W_l + bias) for every b, so
    //   dW_l = ELU'(W_l + bias) * (1/D_exam) * sum_b d exam/d propensity[b,l],  dbias = sum_l dW_l
    const float bias = aux[L];
    float gsum = 0.f, gsq = 0.f;
    for (int l = threadIdx.x; l < L; l += 256) {
      const float z = aux[l] + bias;
      const float g = (tail[ULTR_TAIL_FIXED + l] / D2) * (z > 0.f ? 1.0f : expf(z));
      gsum += g;
      gsq += g * g;
    }
    gsum = block_sum256(gsum, sm);
    gsq = block_sum256(gsq, sm);
    pnorm = sqrtf(gsq + gsum * gsum);
    const float pc = (u.max_gradient_norm > 0.f) ? fminf(1.0f, u.max_gradient_norm / (pnorm + 1e-6f)) : 1.0f;
    for (int l = threadIdx.x; l < L; l += 256) {
      const float z = aux[l] + bias;
      const float g = (tail[ULTR_TAIL_FIXED + l] / D2) * (z > 0.f ? 1.0f : expf(z)) * pc;
      if constexpr (ADAM) {  // the propensity parameters' own moments: m_aux[L + 1] | v_aux[L + 1] behind the ranker's
        float* ma = state + 2 * P;
        float* va = ma + (L + 1);
        float m = ma[l], v = va[l];
        aux[l] = adam_step(aux[l], g, &m, &v, oa.step_aux, oa.rsq2, u.adagrad_eps);
        ma[l] = m;
        va[l] = v;
      } else {
        aux[l] = opt_step(aux[l], g, nullptr, u.optimizer, true, u.propensity_learning_rate, u.adagrad_eps);
      }
    }
    __syncthreads();  // every thread has read the old bias
    if constexpr (ADAM) {
      if (threadIdx.x == 0) {
        float* ma = state + 2 * P;
        float* va = ma + (L + 1);
        float m = ma[L], v = va[L];
        aux[L] = adam_step(bias, gsum * pc, &m, &v, oa.step_aux, oa.rsq2, u.adagrad_eps);
        ma[L] = m;
        va[L] = v;
      }
    } else {
      if (threadIdx.x == 0) aux[L] = opt_step(bias, gsum * pc, nullptr, u.optimizer, true, u.propensity_learning_rate, u.adagrad_eps);
    }
  } else if ((u.algo == ULTR_ALGO_PAIRDEBIAS || u.algo == ULTR_ALGO_LAMBDARANK) && aux != nullptr) {
    // t <- (1 - a) t + a * (t_loss / t_loss[0]) ^ (1 / (p + 1));   LambdaRank divides with _safe_div
    const bool safe = (u.algo == ULTR_ALGO_LAMBDARANK);
    const float ex = 1.0f / (u.regulation_p + 1.0f);
    const float a = u.em_step_size, oma = (float)(1.0 - (double)u.em_step_size);
    const float tp0 = tail[ULTR_TAIL_FIXED], tm0 = tail[ULTR_TAIL_FIXED + L];
    for (int l = threadIdx.x; l < 2 * L; l += 256) {
      const float den = (l < L) ? tp0 : tm0;
      const float num = tail[ULTR_TAIL_FIXED + l];
      const float ratio = (safe && den == 0.f) ? 0.f : num / den;
      const float pw = (ex == 0.5f) ? sqrtf(ratio) : powf(ratio, ex);
      aux[l] = oma * aux[l] + a * pw;
    }
  } else if (u.algo == ULTR_ALGO_REGEM && aux != nullptr) {
    // M-step: propensity <- (1 - a) propensity + a * mean_b(c + (1 - c) P(e=1, r=0 | c=0))   (regression_EM.py:180-183)
    const float a = u.em_step_size, oma = (float)(1.0 - (double)u.em_step_size);
    const float nb = D / (float)L;  // lists in the (global) batch
    for (int l = threadIdx.x; l < L; l += 256) aux[l] = oma * aux[l] + a * (tail[ULTR_TAIL_FIXED + l] / nb);
  } else if (u.algo == ULTR_ALGO_TWOTOWER && aux != nullptr) {
    // the observation tower theta = aux[0 .. L): gradient tail / D, a clip of its own (as DLA's two models), the descriptor's
    // optimizer at propensity_learning_rate with PERSISTENT state behind the ranker's (ultr_opt_state_floats): Adagrad's L
    // accumulators at state[P], Adam's m[L] | v[L] at state[2 P]; the step count is the ranker's
    float gsq = 0.f;
    for (int l = threadIdx.x; l < L; l += 256) {
      const float g = tail[ULTR_TAIL_FIXED + l] / D;
      gsq += g * g;
    }
    gsq = block_sum256(gsq, sm);
    pnorm = sqrtf(gsq);
    const float pc = (u.max_gradient_norm > 0.f) ? fminf(1.0f, u.max_gradient_norm / (pnorm + 1e-6f)) : 1.0f;
    for (int l = threadIdx.x; l < L; l += 256) {
      const float g = (tail[ULTR_TAIL_FIXED + l] / D) * pc;
      if constexpr (ADAM) {
        float* ma = state + 2 * P;
        float* va = ma + L;
        float m = ma[l], v = va[l];
        aux[l] = adam_step(aux[l], g, &m, &v, oa.step_aux, oa.rsq2, u.adagrad_eps);
        ma[l] = m;
        va[l] = v;
      } else {
        float* acc = (state != nullptr && u.optimizer != ULTR_OPT_SGD) ? state + P + l : nullptr;
        aux[l] = opt_step(aux[l], g, acc, u.optimizer, acc == nullptr, u.propensity_learning_rate, u.adagrad_eps);
      }
    }
  }
  if (threadIdx.x == 0 && scalars_out != nullptr) {
    scalars_out[0] = loss;
    scalars_out[1] = norm;
    scalars_out[2] = coef;
    scalars_out[3] = D;
    scalars_out[4] = rank_loss;
    scalars_out[5] = exam_loss;
    scalars_out[6] = pnorm;
    scalars_out[7] = ss;
  }
  if (threadIdx.x == 0 && u.host_scalars != nullptr) {
    const float v[8] = {loss, norm, coef, D, rank_loss, exam_loss, pnorm, ss};
    // a weight outside the range of the split-half copies (DnnPlan::h3_flag_off: raised by the build kernel or by an earlier
    // update launch - this launch's own tiles report with the next step): the host's read of the loss raises
    uint32_t st = 0u;
    if (h3flag != nullptr) {
      const uint32_t f = __hip_atomic_load(h3flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st = ((f & ULTR_H3_FLAG_OVER) ? ULTR_STATUS_H3_RANGE : 0u) | ((f & ULTR_H3_FLAG_NEAR) ? ULTR_STATUS_H3_NEAR : 0u);
    }
    host_report(u, v, st);
  }
}

template <bool ADAM>
__global__ __launch_bounds__(256) void update_kernel(ultr_update_desc u, DnnPlan dp, float* __restrict__ params,
                                                     float* __restrict__ state, const float* __restrict__ grads,
                                                     float* __restrict__ aux, const float* __restrict__ sumsq_part, int nsq,
                                                     float* __restrict__ scalars_out, const float* __restrict__ l2_sums, int nsq2,
                                                     OptArgs<ADAM> oa) {
  if (update_guarded(u)) return;
  // flat variant (no k-major copy to maintain): one element per thread, loads issued BEFORE the norm reduction so
  // that the two memory round trips overlap
  __shared__ float sm[4];
  const int64_t P = u.n_params;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = e < P;
  const int64_t ea[1] = {live ? e : -1};
  const float g_raw[1] = {live ? grads[e] : 0.f};
  const float p_old[1] = {live ? params[e] : 0.f};
  const float s_old[1] = {(live && state != nullptr) ? state[e] : 0.f};
  float v_old[1] = {0.f};
  if constexpr (ADAM) v_old[0] = live ? state[P + e] : 0.f;  // (Adam: s_old is m; the launcher refused a NULL state)
  float ss = 0.f;
  if (nsq2 > 0) {  // level-2 partials of this step's reduction launch (ultr_sumsq2_off)
    const float* s2 = sumsq_part + ultr_sumsq2_off(P);
    for (int k = threadIdx.x; k < nsq2; k += 256) ss += s2[k];
  } else {
    ss = sumsq_level1_as_level2(sumsq_part, nsq, threadIdx.x);
  }
  ss = block_sum256(ss, sm);
  float pn[1];
  update_body<1, ADAM>(u, dp, params, state, grads + P, aux, ss, ea, g_raw, p_old, s_old, v_old, oa, pn, sm, scalars_out, l2_sums,
                       u.range_flag);
}

// The update's work map (DnnPlan::upd_* / vs_* and the K, M, off_w of the layers) in LDS.  DnnPlan is a by-value kernel
// argument of 1.6 KB and the argument segment is rewritten by every launch: the old head chained runtime-indexed reads of it
// (upd_tile_begin[nl - 1], the `while` over upd_tile_begin[j + 1], upd_ntk[j], M[j], K[j], off_w[j]; per THREAD over vs_begin[] in
// the vector workgroups), each on another cold line and each waiting for the one before, ahead of the first gradient word.
// update_tiled_kernel copies two pieces of the plan - words [0, UPD_A_DW): nl .. off_w[], and [UPD_B0, UPD_B0 + UPD_B_DW):
// upd_tile_begin .. vs_begin[] - with one load per thread and searches the copy.
#define UPD_A_DW ((int)(offsetof(DnnPlan, off_b) / 4))
#define UPD_B0 ((int)(offsetof(DnnPlan, upd_tile_begin) / 4))
#define UPD_B_DW ((int)(offsetof(DnnPlan, fwd_ksplit) / 4) - UPD_B0)
static_assert(UPD_A_DW + UPD_B_DW <= 256, "one word per thread");
static_assert(offsetof(DnnPlan, off_w) < offsetof(DnnPlan, off_b) && offsetof(DnnPlan, M) < offsetof(DnnPlan, off_b) &&
              offsetof(DnnPlan, upd_ntk) > offsetof(DnnPlan, upd_tile_begin) && offsetof(DnnPlan, vs_begin) < offsetof(DnnPlan, fwd_ksplit) &&
              offsetof(DnnPlan, vs_off) > offsetof(DnnPlan, upd_tile_begin) && offsetof(DnnPlan, vs_pv) < offsetof(DnnPlan, fwd_ksplit),
              "the staged pieces hold every field the head reads");
// index of the staged copy of the word at byte `off` of DnnPlan
__device__ __forceinline__ constexpr int upd_at(size_t off) {
  return (int)(off / 4) < UPD_A_DW ? (int)(off / 4) : UPD_A_DW + (int)(off / 4) - UPD_B0;
}
// element j (workgroup-uniform) of an int / int64 array of the plan, as a scalar
__device__ __forceinline__ int upd_u(const int* sm_plan, size_t off, int j) {
  return __builtin_amdgcn_readfirstlane(sm_plan[upd_at(off) + j]);
}
__device__ __forceinline__ int64_t upd_u64(const int* sm_plan, size_t off, int j) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane(sm_plan[upd_at(off) + 2 * j]);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane(sm_plan[upd_at(off) + 2 * j + 1]);
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// Variant that keeps the k-major weight copy and the vector-parameter image current (DnnPlan::wt_*).  Workgroups
// [0, n_tiles): one 16x16 tile of a hidden W_j - thread (r, c) updates W_j[m0 + r][k0 + c] (64-byte row segments) and
// the tile goes out transposed through LDS as WT_j[k0 + r][m0 + c] (64-byte segments again; a per-element scatter wrote
// 4 bytes per 64-byte sector: 3.5 MB of write traffic for 0.4 MB of data and ~1 us of the kernel).  The remaining
// workgroups walk the vector parameters segment by segment and write the image.
// TPW tiles (or 256-element pieces of the vector parameters) per workgroup: every workgroup re-sums ALL sum-of-squares
// partials (one per 64 parameters) for its copy of the clip coefficient - at 0.5 M parameters (config 4) that is 32 KB per
// workgroup and 2050 workgroups; four units per workgroup quarter that traffic (update 14 -> 8 us there).
template <int TPW, bool ADAM>
__global__ __launch_bounds__(256) void update_tiled_kernel(ultr_update_desc u, DnnPlan dp, float* __restrict__ params,
                                                           float* __restrict__ state, const float* __restrict__ grads,
                                                           float* __restrict__ aux, float* __restrict__ wt,
                                                           const float* __restrict__ sumsq_part, int nsq,
                                                           float* __restrict__ scalars_out, int n_tile_blocks,
                                                           const float* __restrict__ l2_sums, int nsq2, int rider_first, ultr_click_args rider,
                                                           OptArgs<ADAM> oa) {
  __shared__ float sm[4];
  __shared__ float tile[TPW][16][17];
  __shared__ int sm_plan[UPD_A_DW + UPD_B_DW];
  // workgroups behind the update's own: the click draw of the NEXT batch (ultr_feed_train_step) - independent of the update, and of
  // its guard (a feed keeps drawing when a data-parallel step was refused)
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15, lane = tid & 63;
  UPD_STAMP(0);
  // the work map -> LDS (upd_at): one word per thread, address = threadIdx only, in the same round trip as the scalar arguments -
  // ahead of the role split and the guard, so that nothing before this load waits for another argument
  const int pw = reinterpret_cast<const int*>(&dp)[tid < UPD_A_DW ? tid : tid < UPD_A_DW + UPD_B_DW ? UPD_B0 + tid - UPD_A_DW : 0];
  // (... and so are the scalar arguments of the head: named here, all of them are fetched now instead of one wait after the other)
  asm volatile("" ::"s"(rider_first), "s"(u.guard), "s"(u.n_params), "s"(dp.nl), "s"(dp.n_vs), "s"(n_tile_blocks), "s"(grads), "s"(params),
               "s"(state), "s"(sumsq_part), "s"(nsq), "s"(nsq2),
               "v"(pw));  // (the staged word is an operand too: its load cannot be scheduled behind the wait for the scalars)
  if (tid < UPD_A_DW + UPD_B_DW) sm_plan[tid] = pw;
  if ((int)blockIdx.x >= rider_first) {
    click_draw(rider, (int)blockIdx.x - rider_first);
    return;
  }
  if (update_guarded(u)) return;
  const int64_t P = u.n_params;
  __syncthreads();
  const int nl = dp.nl;
  const int tbeg = sm_plan[upd_at(offsetof(DnnPlan, upd_tile_begin)) + (lane & 15)];  // lane i: first tile of layer i, i <= ULTR_MAXL
  const int n_tiles = __builtin_amdgcn_readlane(tbeg, nl - 1);
  int64_t ea[TPW];
  int jj[TPW], m0[TPW], k0[TPW], pvpos[TPW];
  const bool is_tile = (int)blockIdx.x < n_tile_blocks;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    ea[q] = -1; jj[q] = -1; m0[q] = 0; k0[q] = 0; pvpos[q] = -1;
    if (is_tile) {
      const int tb = (int)blockIdx.x * TPW + q;
      if (tb < n_tiles) {
        // the layer of tile tb: lane i compares with layer i's first tile; the leading ones from layer 1 on are what
        // `while (j + 1 < nl - 1 && tb >= upd_tile_begin[j + 1]) ++j` counted
        const unsigned long long bal = __ballot(lane >= 1 && lane < nl - 1 && tb >= tbeg);
        const int j = __builtin_ctzll(~(bal >> 1));
        const int t = tb - __builtin_amdgcn_readlane(tbeg, j);
        const int ntk = upd_u(sm_plan, offsetof(DnnPlan, upd_ntk), j);
        const int Mj = upd_u(sm_plan, offsetof(DnnPlan, M), j), Kj = upd_u(sm_plan, offsetof(DnnPlan, K), j);
        const int64_t ow = upd_u64(sm_plan, offsetof(DnnPlan, off_w), j);
        const int tm = t / ntk;
        jj[q] = j;
        m0[q] = tm * 16;
        k0[q] = (t - tm * ntk) * 16;
        if (m0[q] + r < Mj && k0[q] + c < Kj) ea[q] = ow + (int64_t)(m0[q] + r) * Kj + k0[q] + c;
      }
    } else {
      // vector parameters: the segments the workgroup's 256 elements touch are [s0, s1] (two ballots over the segment starts,
      // as in the slab reduction's red_lookup); a thread advances from s0 by uniform-address LDS reads
      const int n_vs = dp.n_vs;
      const int vs_begin = upd_at(offsetof(DnnPlan, vs_begin));
      const int n_vec = sm_plan[vs_begin + n_vs];
      const int v0 = (((int)blockIdx.x - n_tile_blocks) * TPW + q) * 256, v = v0 + tid;
      const int v1 = v0 + 255 < n_vec ? v0 + 255 : n_vec - 1;
      const int vb = sm_plan[vs_begin + (lane < 2 * ULTR_MAXL + 2 ? lane : 2 * ULTR_MAXL + 2)];
      const bool in = lane >= 1 && lane < n_vs;
      const unsigned long long b0 = __ballot(in && v0 >= vb), b1 = __ballot(in && v1 >= vb);
      const int s0 = __builtin_ctzll(~(b0 >> 1)), s1 = __builtin_ctzll(~(b1 >> 1));
      int sg = s0;
      bool ok = true;
      for (int i = s0 + 1; i <= s1; ++i) {
        ok = ok && v >= sm_plan[vs_begin + i];
        sg += ok ? 1 : 0;
      }
      if (v < n_vec) {
        const int at = upd_at(offsetof(DnnPlan, vs_off)) + 2 * sg;
        const int64_t vo = (int64_t)(((unsigned long long)(unsigned)sm_plan[at + 1] << 32) | (unsigned)sm_plan[at]);
        const int d = v - sm_plan[vs_begin + sg];
        ea[q] = vo + d;
        pvpos[q] = sm_plan[upd_at(offsetof(DnnPlan, vs_pv)) + sg] + d;
      }
    }
  }
  UPD_AFTER((int)ea[0]);
  UPD_STAMP(1);
  float g_raw[TPW], p_old[TPW], s_old[TPW], v_old[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const bool live = ea[q] >= 0;
    g_raw[q] = live ? grads[ea[q]] : 0.f;
    p_old[q] = live ? params[ea[q]] : 0.f;
    s_old[q] = (live && state != nullptr) ? state[ea[q]] : 0.f;
    v_old[q] = 0.f;
    if constexpr (ADAM) v_old[q] = live ? state[P + ea[q]] : 0.f;  // (Adam: s_old is m; the launcher refused a NULL state)
  }
#ifdef ULTR_TRACE
  UPD_AFTER(g_raw[0] + p_old[0] + s_old[0]);
  UPD_STAMP(2);
#endif
  float ss = 0.f;
  if (nsq2 > 0) {  // level-2 partials of this step's reduction launch (ultr_sumsq2_off): a quarter of the words every workgroup reads
    const float* s2 = sumsq_part + ultr_sumsq2_off(P);
    for (int k = tid; k < nsq2; k += 256) ss += s2[k];
  } else {
    ss = sumsq_level1_as_level2(sumsq_part, nsq, tid);
  }
  ss = block_sum256(ss, sm);
  UPD_AFTER(ss);
  UPD_STAMP(3);
  float pn[TPW];
  // block 0's extra duties (EM / propensity updates, step scalars) run inside update_body and need all 256 threads
  if (blockIdx.x != 0) {
    update_body<TPW, ADAM>(u, dp, params, state, grads + P, aux, ss, ea, g_raw, p_old, s_old, v_old, oa, pn, sm, nullptr, l2_sums);
  } else {
    update_body<TPW, ADAM>(u, dp, params, state, grads + P, aux, ss, ea, g_raw, p_old, s_old, v_old, oa, pn, sm, scalars_out, l2_sums,
                     // (only a model whose weights some split-half product may READ reports: with the knobs off, or for a model
                     // switched to the fp32 products, a large weight is harmless)
                     (dp.h3_flag_off > 0 && dp.h3_watch) ? reinterpret_cast<const uint32_t*>(wt + dp.h3_flag_off) : u.range_flag);
  }
  if (is_tile) {
    // range of EVERY hidden weight (not only of the layers with fragment copies: the per-layer big-batch path builds split-half planes
    // of any hidden layer): |w| >= 64 raises NEAR, >= 128 (or NaN) OVER - reported with the next step
    if (dp.h3_flag_off > 0) {
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const float aw = fabsf(pn[q]) * ULTR_H3_WSCALE;
        if (ea[q] >= 0 && !(aw < ULTR_H3_WNEAR))
          flag_or(reinterpret_cast<uint32_t*>(wt + dp.h3_flag_off), !(aw < ULTR_H3_WMAX) ? (ULTR_H3_FLAG_OVER | ULTR_H3_FLAG_NEAR) : ULTR_H3_FLAG_NEAR);
      }
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) tile[q][r][c] = pn[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      const int j = jj[q];
      if (j < 0) continue;
      const int k = k0[q] + r, m = m0[q] + c;  // transposed ownership
      if (k < dp.K[j] && m < dp.M[j]) wt[dp.wt_off[j] + (int64_t)k * dp.M[j] + m] = tile[q][c][r];
      if ((dp.h3f[j] | dp.h3b[j]) && tid >= 128) {
        // the split-half copies (DnnPlan::whf_off / whb_off, ultr_h3_index): the 16 x 16 tile is 64 pieces of 8 halves (16 bytes)
        // of each: 2 planes x 2 quarter-steps x 2 column tiles x 8 lanes; threads 128..191 write the forward copy, 192..255 the
        // dgrad copy
        const int t6 = tid & 63, hl = t6 >> 5, qq = (t6 >> 4) & 1, tt = (t6 >> 3) & 1, jj = t6 & 7;
        const bool fwd = tid < 192;
        if (fwd ? dp.h3f[j] != 0 : dp.h3b[j] != 0) {
          // forward: output column = m (tile row), contraction = k (tile column); dgrad: the other way round
          const int c0 = fwd ? m0[q] : k0[q], z0 = fwd ? k0[q] : m0[q];
          const int nks = ((fwd ? dp.K[j] : dp.M[j]) + 31) >> 5;
          const int col = 2 * jj + tt;  // output column inside the tile
          typedef _Float16 h8v __attribute__((ext_vector_type(8)));
          h8v piece;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float w = (fwd ? tile[q][col][8 * qq + e] : tile[q][8 * qq + e][col]) * ULTR_H3_WSCALE;
            const _Float16 hi = (_Float16)w;
            piece[e] = hl ? (_Float16)(w - (float)hi) : hi;
          }
          const int64_t pos = ((((int64_t)(c0 >> 5) * nks + (z0 >> 5)) * 4 + (2 * tt + hl)) * 64 +
                               ((((z0 & 31) >> 3) + qq) * 16 + ((c0 & 31) >> 1) + jj)) * 8;
          _Float16* dst = reinterpret_cast<_Float16*>(wt + (fwd ? dp.whf_off[j] : dp.whb_off[j]));
          *reinterpret_cast<h8v*>(dst + pos) = piece;
        }
      }
      if (dp.sw_ok && tid < 128) {
        // the fragment-major copies (DnnPlan::wsf_off / wsb_off): the 16 x 16 tile is 64 float4 pieces of each, 8 pieces
        // (128 bytes) contiguous; threads 0..63 write the forward copy, 64..127 the dgrad copy (layers >= 1).  Elements
        // beyond K are zero in the tile (and M is a multiple of 32), as the padding of the copies requires.
        const int t6 = tid & 63, uu = t6 >> 5, qq = (t6 >> 3) & 3, ii = t6 & 7;
        const int a = 4 * qq + 2 * uu, b = 2 * ii;  // a: contraction offset inside the tile, b: output-column offset
        if (tid < 64) {
          const int h = (k0[q] & 31) >> 4, ntr = (dp.K[j] + 31) >> 5;
          const int64_t pos = ((((int64_t)(m0[q] >> 5) * ntr + (k0[q] >> 5)) * 4 + (2 * h + uu)) * 64 +
                               (qq * 16 + ((m0[q] & 31) >> 1) + ii)) * 4;
          st4(wt + dp.wsf_off[j] + pos, make_float4(tile[q][b][a], tile[q][b + 1][a], tile[q][b][a + 1], tile[q][b + 1][a + 1]));
        } else if (j >= 1) {
          const int h = (m0[q] & 31) >> 4, ntr = (dp.M[j] + 31) >> 5;
          const int64_t pos = ((((int64_t)(k0[q] >> 5) * ntr + (m0[q] >> 5)) * 4 + (2 * h + uu)) * 64 +
                               (qq * 16 + ((k0[q] & 31) >> 1) + ii)) * 4;
          st4(wt + dp.wsb_off[j] + pos, make_float4(tile[q][a][b], tile[q][a][b + 1], tile[q][a + 1][b], tile[q][a + 1][b + 1]));
        }
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < TPW; ++q)
      if (pvpos[q] >= 0) wt[dp.wt_pv_off + pvpos[q]] = pn[q];
  }
  UPD_STAMP(4);
}

// an ultr_algo value: 0 .. ULTR_ALGO_DBGD, ULTR_ALGO_TWOTOWER, ULTR_ALGO_PLRANK and ULTR_ALGO_AFFINE - the 8 and the 10 between them
// are none (include/ultr_hip.h)
static bool algo_known(int32_t algo) {
  return (algo >= 0 && algo <= ULTR_ALGO_DBGD) || algo == ULTR_ALGO_TWOTOWER || algo == ULTR_ALGO_PLRANK || algo == ULTR_ALGO_AFFINE;
}

extern "C" int64_t ultr_opt_state_floats(const ultr_update_desc* u) {
  if (!u || u->n_params <= 0 || u->list_size <= 0 || !algo_known(u->algo)) return -1;
  const int64_t L = u->list_size;
  const bool tower = u->algo == ULTR_ALGO_TWOTOWER;  // its observation tower keeps optimizer state of its own behind the ranker's
  switch (u->optimizer) {
    case ULTR_OPT_SGD: return 0;
    case ULTR_OPT_ADAGRAD: return u->n_params + (tower ? L : 0);
    case ULTR_OPT_ADAM: return 2 * u->n_params + (u->algo == ULTR_ALGO_DLA ? 2 * (L + 1) : tower ? 2 * L : 0);
  }
  return -1;
}

int ultr_update_check_opt(const ultr_update_desc* u, const float* state) {
  if (u->optimizer != ULTR_OPT_ADAGRAD && u->optimizer != ULTR_OPT_SGD && u->optimizer != ULTR_OPT_ADAM) return ULTR_E_BADARG;
  if (u->optimizer == ULTR_OPT_ADAM && (!state || u->adam_t == 0u)) return ULTR_E_BADARG;
  return 0;
}

// the three kernels of one optimizer class and their launch; the Adagrad / SGD class is the code as it was before Adam
template <bool ADAM>
static void launch_update(UltrProfScope& prof, const ultr_update_desc* u, const DnnPlan& dp, float* params, float* wt, float* state,
                          const float* grads, float* aux, const void* bwd_ws, int nsq, float* scalars_out, const float* l2_sums, int nsq2,
                          const ultr_click_args& rider, int rider_blocks, const OptArgs<ADAM>& oa, void* stream) {
  if (wt != nullptr) {
    const int n_tiles = dp.upd_tile_begin[dp.nl - 1], n_vec = dp.vs_begin[dp.n_vs];
    if (n_tiles + (n_vec + 255) / 256 < 1536) {  // one unit per workgroup keeps the launch wide (config 2: 401 units, config 3: 940 -
                                                 // four per workgroup left 235 workgroups for 256 CUs: 7.0 -> 9.0 us)
      const int own = n_tiles + (n_vec + 255) / 256;
      ULTR_LAUNCH(prof, (update_tiled_kernel<1, ADAM>), dim3(own + rider_blocks), dim3(256), 0, (hipStream_t)stream, *u, dp, params, state,
                  grads, aux, wt, (const float*)bwd_ws, nsq, scalars_out, n_tiles, l2_sums, nsq2, own, rider, oa);
    } else {
      const int tb = (n_tiles + 3) / 4;
      const int own = tb + (n_vec + 1023) / 1024;
      ULTR_LAUNCH(prof, (update_tiled_kernel<4, ADAM>), dim3(own + rider_blocks), dim3(256), 0, (hipStream_t)stream, *u, dp, params, state,
                  grads, aux, wt, (const float*)bwd_ws, nsq, scalars_out, tb, l2_sums, nsq2, own, rider, oa);
    }
  } else {
    const int nblk = (int)((u->n_params + 255) / 256);
    ULTR_LAUNCH(prof, update_kernel<ADAM>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, *u, dp, params, state, grads, aux,
                (const float*)bwd_ws, nsq, scalars_out, l2_sums, nsq2, oa);
  }
}

extern "C" int ultr_apply_update(const ultr_update_desc* u, const ultr_dnn_desc* d, float* params, float* wt, float* state,
                                 const float* grads, float* aux, const void* bwd_ws, float* scalars_out, void* stream) {
  return ultr_apply_update_ex(u, d, params, wt, state, grads, aux, bwd_ws, scalars_out, 0, nullptr, stream);
}
// nsq2 > 0: the step's slab-reduction launch left level-2 sum-of-squares partials (ultr_plan.h) - library-internal (ultr_train_step)
int ultr_apply_update_ex(const ultr_update_desc* u, const ultr_dnn_desc* d, float* params, float* wt, float* state, const float* grads,
                         float* aux, const void* bwd_ws, float* scalars_out, int nsq2, const ultr_click_args** rider_io, void* stream) {
  if (!u || !params || !grads || !bwd_ws || u->n_params <= 0 || u->list_size <= 0) return ULTR_E_BADARG;
  if (!ultr_aligned16(wt)) return ULTR_E_BADARG;  // update_tiled_kernel writes the copies with 16-byte stores (the operand contract, ultr_plan.h)
  DnnPlan dp;
  memset(&dp, 0, sizeof(dp));
  if (wt != nullptr) {
    if (!ultr_make_dnn_plan(d, 0, &dp) || dp.P != u->n_params) return ULTR_E_BADARG;
  }
  if (!algo_known(u->algo) || ultr_update_check_opt(u, state)) return ULTR_E_BADARG;
  if (u->algo != ULTR_ALGO_SOFTMAX && u->algo != ULTR_ALGO_PRS && u->algo != ULTR_ALGO_PDGD && u->algo != ULTR_ALGO_DBGD &&
      u->algo != ULTR_ALGO_PLRANK && u->algo != ULTR_ALGO_AFFINE && !aux)
    return ULTR_E_BADARG;
  if (u->optimizer == ULTR_OPT_ADAGRAD && u->algo != ULTR_ALGO_DLA && !state) return ULTR_E_BADARG;
  if (u->l2_loss < 0.f || (u->l2_loss > 0.f && !scalars_out) ||
      (u->l2_loss > 0.f && (u->algo == ULTR_ALGO_LAMBDARANK || u->algo == ULTR_ALGO_PRS || u->algo == ULTR_ALGO_DBGD)))
    return ULTR_E_BADARG;  // LambdaRank and PRSrank have no l2_loss hyper-parameter (lambda_rank.py:42-49, prs_rank.py:43-50)
  const int tail = (int)ultr_tail_len(u->list_size);
  const int nsq = (int)ultr_red_blocks(u->n_params, tail);
  const float* l2_sums = nullptr;
  if (u->l2_loss > 0.f) {
    hipLaunchKernelGGL(l2_sums_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)params, grads, u->n_params,
                       scalars_out + 8);
    l2_sums = scalars_out + 8;
  }
  UltrProfScope prof(ULTR_K_UPDATE, (hipStream_t)stream);
  // a click draw waiting for a launch to ride on (ultr_feed_train_step): its (batch + 3) / 4 workgroups follow the update's
  ultr_click_args rider;
  memset(&rider, 0, sizeof(rider));
  int rider_blocks = 0;
  if (wt != nullptr && rider_io != nullptr && *rider_io != nullptr) {
    rider = **rider_io;
    rider_blocks = (rider.batch + 3) / 4;
    *rider_io = nullptr;
  }
  if (u->optimizer == ULTR_OPT_ADAM)
    launch_update<true>(prof, u, dp, params, wt, state, grads, aux, bwd_ws, nsq, scalars_out, l2_sums, nsq2, rider, rider_blocks,
                        adam_corr(*u), stream);
  else
    launch_update<false>(prof, u, dp, params, wt, state, grads, aux, bwd_ws, nsq, scalars_out, l2_sums, nsq2, rider, rider_blocks,
                         OptArgs<false>(), stream);
  return (int)hipGetLastError();
}
