// ultr_dbgd.hip - the weight-perturbing online learners DBGD and MGD (reference dbgd.py:125-330, mgd.py:86-232,
// team_draft_interleave.py): candidate noise, team-draft multileaving with simulated clicks, and the gradient of the winners.
//
// A step of R candidates (R = 1: DBGD, R = ranker_num: MGD; ranker 0 is the current model) is, on one stream:
//   dbgd_noise_kernel       u_r = F.normalize(N(0, 1), dim = 0) per Linear parameter (per input column of a weight, over the whole
//                           bias; the [1, in] scorer row becomes sign(z)), 0 on the LayerNorm entries; theta_r = theta + noise_rate u_r
//   R + 1 validation forwards of the caller (ultr_dnn_forward, one per parameter vector) into scores [R + 1, B, L]
//   dbgd_interleave_kernel  (need_interleave) per list, one wavefront: list_len, each ranker's order (ultr_rank.h: the online feeds'
//                           stable sort or Plackett-Luce race), the team-draft multileave, clicks on the first
//                           min(list_len, rank_list_size) positions redrawn while the list has none, winners [B, R + 1]
//   ultr_ndcg of the caller (the loss 1 - NDCG@rank_list_size of the current model; without interleaving: every ranker's NDCG)
//   dbgd_grad_kernel        grads = -sum_r c_r u_r (the update steps TOWARD the winners), the step tail with the loss, and the
//                           sum-of-squares partials ultr_apply_update reads
//   ultr_apply_update of the caller (clip + SGD / Adagrad, algo ULTR_ALGO_DBGD)
// Randomness: Philox-4x32-10 keyed by (seed, step); counters (element, ranker, 0, NOISE) for the normals, (list, ranker, l / 4, RACE)
// for the race, (list, round, t / 4, SHUFFLE) for the team shuffles and (list, attempt, l / 4, CLICK) for the clicks.  A step is a
// pure function of (seed, step, parameters, batch), independent of the launch geometry.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_click.h"
#include "ultr_dbgd.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_rank.h"

#define DBGD_NOISE_TAG 0x0DB6D001u
#define DBGD_RACE_TAG 0x0DB6D002u
#define DBGD_SHUFFLE_TAG 0x0DB6D003u
#define DBGD_CLICK_TAG 0x0DB6D004u
#define DBGD_NORM_EPS 1e-12f  // F.normalize's eps

// the standard normal of element e of ranker r (ultr_dbgd.h)
__device__ __forceinline__ float dbgd_normal(const ultr_dbgd_args& a, const Philox& rng, int r, int64_t e) {
  if (a.noise_in != nullptr) return a.noise_in[(int64_t)r * a.n_params + e];
  return philox_normal(rng, r, e, DBGD_NOISE_TAG);
}

// grid (sum_j tiles[j], R), 1024 threads.  A column tile of W_j [M_j, K_j]: 16 columns (lane & 15), 64 row phases (4 per wave), rows
// phase, phase + 64, ...; the column norm is reduced in LDS in a fixed order (phase 0, 1, ...) and the normals are generated again for
// the second pass (no scratch buffer).  The last workgroup of a layer: the bias (one vector norm) and the zeros of the LayerNorm
// gamma / beta.
__global__ __launch_bounds__(1024) void dbgd_noise_kernel(ultr_dbgd_args a, DbgdLayout ly) {
  __shared__ float sm[64][DBGD_TILE_COLS];
  const int r = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const Philox rng = philox_step_key(a.seed, a.step);
  const int64_t P = ly.P;
  float* __restrict__ u = a.noise + (int64_t)r * P;
  float* __restrict__ th = a.cand_params + (int64_t)r * (a.cand_stride > 0 ? a.cand_stride : P);
  const float rate = a.noise_rate;
  int j = 0, t = blockIdx.x;
  while (j < ly.nl - 1 && t >= ly.tiles[j]) t -= ly.tiles[j++];
  const int K = ly.K[j], M = ly.M[j];
  if (t < ly.tiles[j] - 1) {
    const int cl = lane & (DBGD_TILE_COLS - 1), ph = w * 4 + (lane >> 4);
    const int c = t * DBGD_TILE_COLS + cl;
    const bool live = c < K;
    float ss = 0.f;
    if (live)
      for (int o = ph; o < M; o += 64) {
        const float z = dbgd_normal(a, rng, r, ly.off_w[j] + (int64_t)o * K + c);
        ss += z * z;
      }
    sm[ph][cl] = ss;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < 64; ++k) s += sm[k][cl];
    const float den = fmaxf(sqrtf(s), DBGD_NORM_EPS);
    if (live)
      for (int o = ph; o < M; o += 64) {
        const int64_t e = ly.off_w[j] + (int64_t)o * K + c;
        const float v = dbgd_normal(a, rng, r, e) / den;
        u[e] = v;
        th[e] = a.params[e] + rate * v;
      }
  } else {
    float ss = 0.f;
    for (int o = threadIdx.x; o < M; o += 1024) {
      const float z = dbgd_normal(a, rng, r, ly.off_b[j] + o);
      ss += z * z;
    }
    ss = wave_sum(ss);
    if (lane == 0) sm[w][0] = ss;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < 16; ++k) s += sm[k][0];
    const float den = fmaxf(sqrtf(s), DBGD_NORM_EPS);
    for (int o = threadIdx.x; o < M; o += 1024) {
      const int64_t e = ly.off_b[j] + o;
      const float v = dbgd_normal(a, rng, r, e) / den;
      u[e] = v;
      th[e] = a.params[e] + rate * v;
    }
    for (int k = threadIdx.x; k < 2 * K; k += 1024) {  // LayerNorm weight and bias: no noise
      const int64_t e = ly.off_ln[j] + k;
      u[e] = 0.f;
      th[e] = a.params[e];
    }
  }
}

// one wavefront per list
__global__ __launch_bounds__(64) void dbgd_interleave_kernel(ultr_dbgd_args a) {
  __shared__ unsigned key[ULTR_DBGD_MAX_M];
  __shared__ uint8_t rk[ULTR_DBGD_MAX_RANKERS][ULTR_DBGD_MAX_M];  // candidate index at each rank, per ranker
  __shared__ int ml[ULTR_DBGD_MAX_M];                              // the multileaved list (candidate indexes)
  __shared__ int tm[ULTR_DBGD_MAX_M];                              // its teams (-1: the agreed prefix)
  __shared__ float ck_s[ULTR_DBGD_MAX_M];
  __shared__ uint8_t placed[ULTR_DBGD_MAX_M];
  __shared__ int idx_s[ULTR_DBGD_MAX_RANKERS], asg_s[ULTR_DBGD_MAX_RANKERS];
  __shared__ float rc_s[ULTR_DBGD_MAX_RANKERS];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int B = a.batch, M = a.max_candidates, NR = a.n_rankers + 1, rls = a.rank_list_size;
  const int32_t pad = (int32_t)a.n_docs;
  const Philox rng = philox_step_key(a.seed, a.step);

  int last = -1;
  for (int l = lane; l < M; l += 64)
    if (a.docids[(int64_t)l * B + b] != pad) last = l;
  const int len = wave_max_int(last) + 1;
  if (a.loss_scores != nullptr)  // the current model's first rank_list_size scores, [B, rank_list_size], for the loss's NDCG
    for (int l = lane; l < rls; l += 64) a.loss_scores[(int64_t)b * rls + l] = a.scores[(int64_t)b * M + l];

  // every ranker's order of the first list_len candidates
  for (int j = 0; j < NR; ++j) {
    wave_rank_keys(a.scores + ((int64_t)j * B + b) * M, len, a.mode == ULTR_ONLINE_STOCHASTIC, a.tau, rng, (uint32_t)b, (uint32_t)j,
                   DBGD_RACE_TAG, key, lane);
    wave_rank_by_count(key, len, rk[j], lane);
    wave_lds_sync();
  }

  // the prefix on which all rankings agree: team -1 (team_draft_interleave.py:21-26)
  int prefix = len;
  for (int p0 = 0; p0 < len; p0 += 64) {
    const int p = p0 + lane;
    bool differ = false;
    if (p < len)
      for (int j = 1; j < NR; ++j) differ = differ || rk[j][p] != rk[0][p];
    const uint64_t m = __ballot(differ);
    if (m) {
      prefix = p0 + (int)__builtin_ctzll(m);
      break;
    }
  }
  for (int d = lane; d < M; d += 64) placed[d] = 0;
  wave_lds_sync();
  for (int p = lane; p < prefix; p += 64) {
    ml[p] = rk[0][p];
    tm[p] = -1;
    placed[rk[0][p]] = 1;
  }
  wave_lds_sync();

  // the draft (:28-43): a fresh shuffle of the rankers every R + 1 picks, each picked ranker adds its best document not yet placed.
  // Sequential by nature: one lane, state in LDS.
  if (lane == 0) {
    for (int j = 0; j < NR; ++j) {
      idx_s[j] = prefix;
      asg_s[j] = j;
    }
    int ai = NR, round = 0;
    for (int p = prefix; p < len; ++p) {
      if (ai == NR) {
        if (a.shuffles_in != nullptr) {
          for (int j = 0; j < NR; ++j) {
            const int v = a.shuffles_in[((int64_t)b * M + round) * NR + j];
            asg_s[j] = (v >= 0 && v < NR) ? v : 0;
          }
        } else {  // Fisher-Yates over the current assignment, as np.random.shuffle does in place
          uint32_t c[4] = {0u, 0u, 0u, 0u};
          for (int i = NR - 1, t = 0; i >= 1; --i, ++t) {
            if ((t & 3) == 0) {
              c[0] = (uint32_t)b;
              c[1] = (uint32_t)round;
              c[2] = (uint32_t)(t >> 2);
              c[3] = DBGD_SHUFFLE_TAG;
              rng(c);
            }
            int s = (int)(u01(c[t & 3]) * (float)(i + 1));
            s = s < i ? s : i;
            const int x = asg_s[i];
            asg_s[i] = asg_s[s];
            asg_s[s] = x;
          }
        }
        ++round;
        ai = 0;
      }
      const int r = asg_s[ai++];
      int i = idx_s[r];
      while (i < len - 1 && placed[rk[r][i]]) ++i;  // (a ranker never runs out: all rankings hold the same documents)
      const int d = rk[r][i];
      ml[p] = d;
      tm[p] = r;
      placed[d] = 1;
      idx_s[r] = i + 1;
    }
  }
  wave_lds_sync();

  // clicks on the labels of the multileaved order (dbgd.py:311-324), redrawn while the list has none
  const int cut = len < rls ? len : rls;
  if (a.clicks_in != nullptr) {
    for (int l = lane; l < cut; l += 64) ck_s[l] = a.clicks_in[(int64_t)l * B + b];
  } else {
    const ClickModel cm = click_model_of(a);
    for (int attempt = 0; attempt <= a.max_redraws && cut > 0; ++attempt)
      if (wave_click_walk(
              cm, rng, (uint32_t)b, (uint32_t)attempt, DBGD_CLICK_TAG, cut, lane, [&](int l) { return a.labels[(int64_t)ml[l] * B + b]; },
              [&](int l, float ck) { ck_s[l] = ck; }) > 0.f)
        break;
  }
  wave_lds_sync();

  // winners (infer_winner, :46-51): clicks of team r / (clicks of all teams + 1e-7); the agreed prefix belongs to no team
  if (lane < NR) {
    float s = 0.f;
    for (int p = 0; p < cut; ++p) s += tm[p] == lane ? ck_s[p] : 0.f;
    rc_s[lane] = s;
  }
  wave_lds_sync();
  if (lane < NR) {
    float tot = 0.f;
    for (int j = 0; j < NR; ++j) tot += rc_s[j];
    a.winners[(int64_t)b * NR + lane] = rc_s[lane] / (tot + 1e-7f);
  }
  for (int p = lane; p < M; p += 64) {
    const int64_t o = (int64_t)p * B + b;
    if (a.interleaved != nullptr) a.interleaved[o] = p < len ? ml[p] : -1;
    if (a.teams != nullptr) a.teams[o] = p < len ? tm[p] : -2;
    if (a.clicks != nullptr) a.clicks[o] = p < cut ? ck_s[p] : 0.f;
  }
}

// grads [P + tail] = -sum_{r >= 1} c_r u_r, the step tail ([0] the loss, [1] D = 1), and one sum-of-squares partial per 64 gradient
// elements (grad_sumsq_kernel's geometry and arithmetic).  c_r (compute_gradient, dbgd.py:196-222 / mgd.py:205-232):
//   need_interleave   mean over the batch of winners[:, r] (fixed-order wave sum)
//   otherwise         the reference broadcasts its [R + 1] winner vector against [1, R + 1, ...]: every ranker's noise is weighted
//                     by the mean of the winners, w = ceil(NDCG_r - NDCG_0) / (sum + 1e-9)
__global__ __launch_bounds__(256) void dbgd_grad_kernel(ultr_dbgd_args a, int64_t total) {
  __shared__ float c_s[ULTR_DBGD_MAX_RANKERS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int R = a.n_rankers, NR = R + 1;
  const int64_t P = a.n_params;
  if (w == 0) {
    if (a.need_interleave) {
      for (int r = 0; r < NR; ++r) {  // lanes over the batch, then the wave's fixed-order sum
        float s = 0.f;
        for (int bb = lane; bb < a.batch; bb += 64) s += a.winners[(int64_t)bb * NR + r];
        s = wave_sum(s);
        if (lane == 0) c_s[r] = s / (float)a.batch;
      }
    } else if (lane == 0) {
      float g[ULTR_DBGD_MAX_RANKERS], sg = 0.f, sw = 0.f;
      for (int r = 0; r < NR; ++r) {
        g[r] = ceilf(a.ndcg[r] - a.ndcg[0]);
        sg += g[r];
      }
      for (int r = 0; r < NR; ++r) sw += g[r] / (sg + 1e-9f);
      for (int r = 0; r < NR; ++r) c_s[r] = sw / (float)NR;
    }
  }
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float gv = 0.f;
  if (e < P) {
    for (int r = 1; r <= R; ++r) gv += c_s[r] * a.noise[(int64_t)(r - 1) * P + e];
    gv = -gv;
    a.grads[e] = gv;
  } else if (e < total) {
    const int k = (int)(e - P);
    a.grads[e] = k == 0 ? 1.0f - a.ndcg[0] : (k == 1 ? 1.0f : 0.f);
  }
  float gg = gv * gv;
  asm volatile("" : "+v"(gg));  // rounded before the first cross-lane add, as in grad_sumsq_kernel
  const float sq = wave_sum(gg);
  const int64_t part = (int64_t)blockIdx.x * 4 + w;
  if (lane == 0 && part < (total + 63) / 64) static_cast<float*>(a.bwd_ws)[part] = sq;
}

extern "C" int ultr_dbgd_noise_args(const ultr_dbgd_args* a, void* stream) {
  DbgdLayout ly;
  if (!dbgd_shape_ok(a) || !a->params || !a->noise || !a->cand_params || !dbgd_layout(a, &ly)) return ULTR_E_BADARG;
  int T = 0;
  for (int j = 0; j < ly.nl; ++j) T += ly.tiles[j];
  hipLaunchKernelGGL(dbgd_noise_kernel, dim3(T, a->n_rankers), dim3(1024), 0, (hipStream_t)stream, *a, ly);
  return (int)hipGetLastError();
}

extern "C" int ultr_dbgd_interleave_args(const ultr_dbgd_args* a, void* stream) {
  if (!dbgd_shape_ok(a) || !a->scores || !a->docids || !a->labels || !a->winners || a->max_redraws < 0 || a->n_docs < 0 ||
      a->n_docs >= ((int64_t)1 << 31) || (a->mode != ULTR_ONLINE_DETERMINISTIC && a->mode != ULTR_ONLINE_STOCHASTIC))
    return ULTR_E_BADARG;
  if (!a->clicks_in && !click_model_ok(click_model_of(*a))) return ULTR_E_BADARG;
  hipLaunchKernelGGL(dbgd_interleave_kernel, dim3(a->batch), dim3(64), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int ultr_dbgd_grad_args(const ultr_dbgd_args* a, void* stream) {
  if (!dbgd_shape_ok(a) || !a->noise || !a->ndcg || !a->grads || !a->bwd_ws || (a->need_interleave && !a->winners))
    return ULTR_E_BADARG;
  const int64_t total = a->n_params + ultr_tail_len(a->max_candidates);
  hipLaunchKernelGGL(dbgd_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a, total);
  return (int)hipGetLastError();
}
