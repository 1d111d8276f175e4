// ultr_online.hip — device-resident online simulation: query pick + candidate gather, then re-rank + clicks
// (reference stochastic_online_simulation_feed.py:96-226, deterministic_online_simulation_feed.py:129-135).
//
// The host online feeds score the batch on the GPU, copy the scores to the host and re-rank / click list by list in Python
// (~15 ms per batch at config 2).  Here the dataset is resident in HBM (ResidentDataset) and a batch is three launches on one
// stream: online_pick_kernel (queries, candidates), the caller's scoring forward of the candidates with the current parameters,
// online_rerank_kernel (the new order and its clicks).  No host synchronisation anywhere.
//
// One wavefront per batch slot, as click_draw.  Per slot of the re-rank:
//   list_len = 1 + the last non-PAD position (interior PADs take part with their score, the model's score of the zero row);
//   keys: deterministic - the score as an unsigned order key (rank_order_key: NaN above +inf, -0 == +0);
//         stochastic    - the exponential race tau (s - max) - log E, E = -log(1 - u) ~ Exp(1): sorting these keys descending
//                         draws a ranking with exactly the Plackett-Luce distribution of sequential sampling without replacement
//                         (np.random.choice(replace=False, p)); a document whose fp32 probability exp(tau (s - max)) / sum is 0
//                         (log p < ln 2^-150) gets key 0, below every drawn one, so those follow in index order (the reference's
//                         `unused` tail);
//   rank by counting over the first list_len keys (ties by index: stable), as ndcg_list_kernel does;
//   clicks on the first min(list_len, rank_list_size) positions of the new order with wave_click_walk (ultr_click.h) - the same
//   per-position decisions as ultr_click_batch - redrawn on the SAME order while the list has no click (check_validation).
// Randomness: Philox-4x32-10 keyed by (seed, step); counters (slot, 0, ~0, QUERY) for the pick, (slot, 0, l / 4, RACE) for the
// race and (slot, attempt, l / 4, CLICK) for the clicks, word l % 4 for position l.  The tags differ from ultr_click_batch's and
// RegressionEM's, so no counter of one stream is a counter of another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_click.h"
#include "ultr_device.h"
#include "ultr_rank.h"

#define ONLINE_MAX_M 256
#define ONLINE_QUERY_TAG 0x0F1A3E01u
#define ONLINE_RACE_TAG 0x0F1A3E02u
#define ONLINE_CLICK_TAG 0x0F1A3E03u

// one workgroup of 256 threads = four batch slots (one per wave)
__global__ __launch_bounds__(256) void online_pick_kernel(ultr_online_args a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int B = a.batch, M = a.max_candidates, lmax = a.lmax;
  if (b >= B) return;
  const Philox rng = philox_step_key(a.seed, a.step);
  uint32_t c[4] = {(uint32_t)b, 0u, 0xFFFFFFFFu, ONLINE_QUERY_TAG};
  rng(c);
  const int64_t n = a.eligible != nullptr ? a.n_eligible : a.n_queries;
  int64_t i = (int64_t)((double)u01(c[0]) * (double)n);
  if (i >= n) i = n - 1;
  int64_t q = a.eligible != nullptr ? (int64_t)a.eligible[i] : i;
  if (q < 0 || q >= a.n_queries) q = 0;  // (an index the caller built wrong must not read out of bounds)
  for (int l = lane; l < M; l += 64) {
    const int32_t d = l < lmax ? a.lists[q * lmax + l] : -1;
    int32_t id = (int32_t)a.n_docs;
    float y = 0.f;
    if (d >= 0) {
      id = d;
      y = a.labels[q * lmax + l];
    }
    a.cand_docids[(int64_t)l * B + b] = id;
    a.cand_labels[(int64_t)l * B + b] = y;
  }
  if (lane == 0 && a.query_idx != nullptr) a.query_idx[b] = (int32_t)q;
}

__global__ __launch_bounds__(256) void online_rerank_kernel(ultr_online_args a) {
  __shared__ unsigned sm_key[4][ONLINE_MAX_M];
  __shared__ int sm_perm[4][ONLINE_MAX_M];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  const int B = a.batch, M = a.max_candidates;
  if (b >= B) return;  // (a whole wave: only wave-level synchronisation below)
  const int32_t pad = (int32_t)a.n_docs;
  unsigned* key = sm_key[w];
  int* perm = sm_perm[w];
  const Philox rng = philox_step_key(a.seed, a.step);

  int last = -1;
  for (int l = lane; l < M; l += 64)
    if (a.cand_docids[(int64_t)l * B + b] != pad) last = l;
  const int len = wave_max_int(last) + 1;

  // keys of the first list_len positions, then the order (ultr_rank.h)
  wave_rank_keys(a.scores + (int64_t)b * M, len, a.mode == ULTR_ONLINE_STOCHASTIC, a.tau, rng, (uint32_t)b, 0u, ONLINE_RACE_TAG, key,
                 lane);
  wave_rank_by_count(key, len, perm, lane);
  for (int i = len + lane; i < M; i += 64) perm[i] = i;
  wave_lds_sync();

  for (int l = lane; l < M; l += 64) {
    const int src = perm[l];
    a.docids[(int64_t)l * B + b] = l < len ? a.cand_docids[(int64_t)src * B + b] : pad;
    if (a.perm != nullptr) a.perm[(int64_t)l * B + b] = src;
  }
  const int cut = len < a.rank_list_size ? len : a.rank_list_size;
  for (int l = cut + lane; l < M; l += 64) a.out_labels[(int64_t)l * B + b] = 0.f;
  if (cut <= 0) return;
  const auto label = [&](int l) { return a.cand_labels[(int64_t)perm[l] * B + b]; };
  const auto store = [&](int l, float ck) { a.out_labels[(int64_t)l * B + b] = ck; };
  if (a.oracle_mode) {  // the clicks are the relevance labels of the new order
    for (int l = lane; l < cut; l += 64) store(l, label(l));
    return;
  }
  const ClickModel cm = click_model_of(a);
  for (int attempt = 0; attempt <= a.max_redraws; ++attempt)  // check_validation: only the clicks are redrawn, on the same order
    if (wave_click_walk(cm, rng, (uint32_t)b, (uint32_t)attempt, ONLINE_CLICK_TAG, cut, lane, label, store) > 0.f) break;
}

static bool online_args_ok(const ultr_online_args* a) {
  return a && a->batch > 0 && a->max_candidates > 0 && a->max_candidates <= ONLINE_MAX_M && a->cand_docids && a->cand_labels &&
         a->n_docs >= 0 && a->n_docs < ((int64_t)1 << 31);
}

extern "C" int ultr_online_pick_args(const ultr_online_args* a, void* stream) {
  if (!online_args_ok(a) || !a->lists || !a->labels || a->n_queries <= 0 || a->lmax <= 0 ||
      (a->eligible != nullptr && a->n_eligible <= 0))
    return ULTR_E_BADARG;
  hipLaunchKernelGGL(online_pick_kernel, dim3((a->batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int ultr_online_rerank_args(const ultr_online_args* a, void* stream) {
  if (!online_args_ok(a) || !a->scores || !a->docids || !a->out_labels || a->rank_list_size < 0 || a->max_redraws < 0 ||
      (a->mode != ULTR_ONLINE_DETERMINISTIC && a->mode != ULTR_ONLINE_STOCHASTIC))
    return ULTR_E_BADARG;
  if (!a->oracle_mode && !click_model_ok(click_model_of(*a))) return ULTR_E_BADARG;
  hipLaunchKernelGGL(online_rerank_kernel, dim3((a->batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
