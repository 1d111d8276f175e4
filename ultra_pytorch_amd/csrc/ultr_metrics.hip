// ultr_metrics.hip — validation-side kernels: padding mask + NDCG@topn, and (ultr_metrics_report) the other seven metrics of the
// reference's factory table from the same ranked list in the same launch.
//
// Replaces BaseAlgorithm.remove_padding_for_metric_eval (reference base_algorithm.py:88-116) and
// ultra.utils.metrics.normalized_discounted_cumulative_gain with weights=None (metrics.py:191-265, 456-495).
// One wavefront per list; the descending sort is rank-by-counting from LDS (stable: ties keep index order,
// which is what torch's CPU sort yields for the all-equal padding scores).  A NaN score ranks above every number, as in torch's
// descending sort, and a NaN in a list becomes the row minimum that its invalid labels take, as torch.min does.
// Lists beyond the 64 KiB of LDS that four such lists share (813 documents) take metrics_long_kernel: one workgroup of 16 waves per list.
//
// ONE ranking core serves both kernels - stage_document, validate_chunk, count_against, place_document, rank_scans, cutoff_sums and
// metrics_means below.  A kernel keeps what is its own: how its threads stride the list, how it reads the keys in the counting loop,
// how it joins the row minimum and the pair count, and how its workgroups arrive at the batch means; the NDCG-only form also keeps
// its batch-mean tail (it measured slower through metrics_means: profiles/metrics_core.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_prof.h"
#include "ultr_rank.h"

#define NDCG_LPW 4
#define NDCG_MAX_TOPN 16

struct TopN {
  int n;
  int v[NDCG_MAX_TOPN];
};
// ultr_ndcg_report: the batch mean inside the SAME launch - the workgroup that arrives last at `counter` sums the per-list values in
// the order ndcg_mean_kernel uses (same bits), writes ndcg_out and, when host != NULL, the values + the sequence number into
// host-mapped memory (what the training step's report does for the loss: the host spins on one word instead of a stream
// synchronisation + device-to-host copy).  counter == NULL: per-list values only (ultr_ndcg's second launch follows).
struct NdcgTail {
  uint32_t* counter;
  float* out;
  float* host;
  uint32_t seq;
};

// ultr_metrics_report (ALL): which metrics, in which order, go into a list's [n][topn.n] block of per_list and of the report
struct MetricSel {
  int n;
  int id[ULTR_MAX_METRICS];
  float pow_max;  // 2^max_label (expected_reciprocal_rank's relevance scale, metrics.py:300-336)
};
#define METRICS_SEQ_WORD (ULTR_MAX_METRICS * NDCG_MAX_TOPN)  // the report's sequence word follows the largest [metrics][topn] block

// LDS bytes of a workgroup: 4 (ALL: 5) [LPW][L] float arrays, ALL: one validity bit per document, the arrival word
static size_t ndcg_lds_bytes(int L, bool all) {
  return all ? ((size_t)NDCG_LPW * 5 * L + (size_t)NDCG_LPW * 2 * ((L + 63) / 64) + 4) * sizeof(float)
             : ((size_t)NDCG_LPW * 4 * L + 4) * sizeof(float);
}

// ---- the ranking core: a list's arrays in LDS are ms (masked + validated predictions, then their order keys, then - ALL - the ERR
// terms by rank), my (validated labels), md / mi (discounted gains by predicted / ideal rank), ALL: ml (validated labels by predicted
// rank) and mv (64-bit masks of the documents whose label was valid: ordered_pair_accuracy counts pairs of those only) ------------------

// document l of list b: pad mask, the masked score out and, with the label, into LDS; the running row minimum and whether a NaN was seen
// (score, doc id and label of a position are requested together: the kernel is a chain of dependent round trips, not bytes)
__device__ __forceinline__ void stage_document(const float* __restrict__ scores, const float* __restrict__ labels,
                                               const int32_t* __restrict__ docids, int64_t n_docs, int B, int L, int b, int l,
                                               float* __restrict__ masked_out, float* ms, float* my, float& mn, bool& nan_seen) {
  float s = scores[(int64_t)b * L + l];
  const float y = labels[(int64_t)l * B + b];
  if (docids != nullptr && (int64_t)docids[(int64_t)l * B + b] == n_docs) s = ULTR_PAD_SCORE;
  if (masked_out != nullptr) masked_out[(int64_t)b * L + l] = s;
  ms[l] = s;
  my[l] = y;
  mn = fminf(mn, s);
  nan_seen = nan_seen || s != s;
}

// the 64-document chunk c, a whole wave (metrics.py:251-264): invalid labels (< 0) -> label 0, prediction rowmin - 1e-6; the validated
// predictions become order keys (rank_order_key) in place.  ALL: the chunk's validity mask into mv
template <bool ALL>
__device__ __forceinline__ void validate_chunk(int c, int L, int lane, float mn, float* ms, float* my, unsigned long long* mv) {
  unsigned* mk = reinterpret_cast<unsigned*>(ms);
  const int l = c * 64 + lane;
  bool ok = false;
  if (l < L) {
    const float y = my[l];
    ok = y >= 0.f;
    my[l] = ok ? y : 0.f;
    mk[l] = rank_order_key(ok ? ms[l] : -1e-6f + mn);
  }
  if constexpr (ALL) {
    const unsigned long long okm = __ballot(ok);
    if (lane == 0) mv[c] = okm;
  }
}

// rank by counting: document d against another one, j - into d's predicted rank rs, its ideal rank ry (ties by index) and, ALL,
// ordered_pair_accuracy's pairs (metrics.py:531-568): label_i > label_j and score_i > score_j, j valid (vj: the mask of j's chunk).
// Between valid documents the keys order as the masked scores compare, but for NaN, which compares false (place_document: i's half)
// (the document and the other one's key and label travel BY VALUE: the conditions stay free of loads, and so free of branches)
struct RankDoc {
  int i;
  unsigned k;
  float y;
};
struct RankCount {
  int rs, ry, pairs;
};
template <bool ALL>
__device__ __forceinline__ void count_against(RankCount& n, RankDoc d, int j, unsigned kj, float yj, unsigned long long vj) {
  n.rs += (kj > d.k || (kj == d.k && j < d.i)) ? 1 : 0;
  n.ry += (yj > d.y || (yj == d.y && j < d.i)) ? 1 : 0;
  if constexpr (ALL) n.pairs += (d.y > yj && d.k > kj && ((vj >> (j & 63)) & 1ull)) ? 1 : 0;
}

// the counted document to its ranks: discounted gains by predicted and by ideal rank, its index into the permutation; ALL: its label by
// predicted rank, and its pairs into this thread's count when it is valid itself and no NaN
template <bool ALL>
__device__ __forceinline__ void place_document(RankDoc d, RankCount n, const unsigned long long* mv, float* ml, float* md, float* mi,
                                               int32_t* __restrict__ order_out, int b, int L, int& opa) {
  if constexpr (ALL) {
    if (((mv[d.i >> 6] >> (d.i & 63)) & 1ull) && d.k != 0xFFFFFFFFu) opa += n.pairs;
    ml[n.rs] = d.y;
  }
  const float gain = exp2f(d.y) - 1.0f;  // weights = 1: gains = 2^label - 1 (metrics.py:213)
  md[n.rs] = gain * (1.0f / log2f((float)n.rs + 2.0f));
  mi[n.ry] = gain * (1.0f / log2f((float)n.ry + 2.0f));
  if (order_out != nullptr) order_out[(int64_t)b * L + n.rs] = d.i;
}

// ONE wave over the labels by predicted rank: the metrics without a cutoff into whole[] (by ULTR_METRIC_* id; the NDCG, DCG and ERR
// entries are filled per cutoff), and the ERR terms by rank into me (over the order keys, which nothing reads any more).  opa_lane:
// this lane's share of the list's correctly ordered pairs (below 2^24 per addend the short kernel passes, one exact addend from the
// long one: the wave sum takes them in lane order either way)
__device__ __forceinline__ void rank_scans(const float* ml, float* me, int L, int lane, float pow_max, float opa_lane,
                                           float (&whole)[ULTR_MAX_METRICS]) {
  float carry = 1.f, ap = 0.f, pos_sum = 0.f, lab_sum = 0.f;  // prod(1 - rel) of the chunks before, sum of precision-at-hit, ARP's sums
  int hits = 0, first = L;                                    // relevant documents so far, the first one's rank
  for (int r0 = 0; r0 < L; r0 += 64) {
    const int r = r0 + lane;
    const float y = r < L ? ml[r] : 0.f;
    const bool hit = r < L && y >= 1.f;
    const float rel = (exp2f(y) - 1.0f) / pow_max;  // metrics.py:320 (0 behind the list's end)
    // the exclusive product of 1 - rel along the rank, formed directly (the reference's cumprod / (1 - rel) is NaN at rel == 1):
    // an inclusive scan over the wave, shifted by one lane, times the carry of the chunks before
    float p = 1.0f - rel;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float t = __shfl_up(p, d);
      if (lane >= d) p *= t;
    }
    float excl = __shfl_up(p, 1);
    if (lane == 0) excl = 1.f;
    excl *= carry;
    carry *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), 63));
    if (r < L) me[r] = rel * excl * (1.0f / (float)(r + 1));
    // mean_average_precision (metrics.py:408-453): hits up to and including this rank / (rank + 1) at every hit
    const unsigned long long hm = __ballot(hit);
    if (hit) ap += (float)(hits + __popcll(hm & ((2ull << lane) - 1ull))) / (float)(r + 1);
    if (first == L && hm != 0) first = r0 + __ffsll((long long)hm) - 1;
    hits += __popcll(hm);
    pos_sum += (float)(r + 1) * y;
    lab_sum += y;
  }
  float sums[4] = {ap, pos_sum, lab_sum, opa_lane};
  wave_sum_n<4>(sums);
  whole[ULTR_METRIC_MRR] = first < L ? 1.0f / (float)(first + 1) : 0.f;
  whole[ULTR_METRIC_MAP] = hits > 0 ? sums[0] / (float)hits : 0.f;
  whole[ULTR_METRIC_ARP] = sums[2] == 0.f ? 0.f : sums[1] / sums[2];  // _safe_div
  whole[ULTR_METRIC_PRECISION] = (float)hits / (float)L;
  whole[ULTR_METRIC_OPA] = sums[3] / ((float)L * (float)L);
  wave_lds_sync();
}

// ONE wave: per cutoff the sums over the ranked arrays and list b's values into per_list.  ALL: the rows sel picks, [sel.n][topn.n],
// written through; otherwise NDCG alone, [topn.n], written through when a batch-mean tail follows in this launch (through)
template <bool ALL>
__device__ __forceinline__ void cutoff_sums(const float* md, const float* mi, const float* me, int L, int lane, int b, int B,
                                            const TopN& topn, const MetricSel& sel, float (&whole)[ULTR_MAX_METRICS],
                                            float* __restrict__ per_list, int width, bool through) {
  for (int k = 0; k < topn.n; ++k) {
    const int n = topn.v[k] < L ? topn.v[k] : L;  // topn clipped to the list size (metrics.py:249)
    float d = 0.f, id = 0.f, e = 0.f;
    for (int r = lane; r < n; r += 64) {
      d += md[r];
      id += mi[r];
      if constexpr (ALL) e += me[r];
    }
    d = wave_sum(d);
    id = wave_sum(id);
    if constexpr (ALL) e = wave_sum(e);
    if (lane == 0) {
      const float v = (id == 0.f) ? 0.f : d / id;  // _safe_div
      if constexpr (ALL) {
        whole[ULTR_METRIC_NDCG] = v;
        whole[ULTR_METRIC_DCG] = d;
        whole[ULTR_METRIC_ERR] = e;
        const Src pl = make_src(per_list, (int64_t)B * width);
        for (int m = 0; m < sel.n; ++m) {
          float x = 0.f;
#pragma unroll
          for (int q = 0; q < ULTR_MAX_METRICS; ++q) x = sel.id[m] == q ? whole[q] : x;  // (registers: no indexed private array)
          coh_st1(pl, (unsigned)(((int64_t)b * width + m * topn.n + k) * 4), x);
        }
      } else if (through) coh_st1(make_src(per_list, (int64_t)B * width), (unsigned)(((int64_t)b * width + k) * 4), v);
      else per_list[(int64_t)b * width + k] = v;
    }
  }
}

// the metric launch's batch means, by the ONE wave that arrived last at tail.counter: lanes stride the lists, fixed-order wave reduction
// per value (ndcg_mean_kernel's order); then the counter is reset and, with a host report, the values and after them the sequence word
// go to host-mapped memory
__device__ __forceinline__ void metrics_means(const float* __restrict__ per_list, int B, int width, int lane, const NdcgTail& tail) {
  const Src pl = make_src(per_list, (int64_t)B * width);
  for (int w = 0; w < width; ++w) {
    float s = 0.f;
    for (int bb = lane; bb < B; bb += 64) s += coh_ld1(pl, (unsigned)(((int64_t)bb * width + w) * 4));  // served from the coherence point
    s = wave_sum(s) / (float)B;
    if (lane == 0) {
      tail.out[w] = s;
      if (tail.host != nullptr) __hip_atomic_store(tail.host + w, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (lane == 0) {
    __hip_atomic_store(tail.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch on this stream
    if (tail.host != nullptr) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(reinterpret_cast<uint32_t*>(tail.host) + METRICS_SEQ_WORD, tail.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ALL = false: NDCG@topn (ultr_ndcg, ultr_ndcg_report).  ALL = true: the same ranking, the same NDCG arithmetic, and the other metrics
// of utils/metrics.py (weights = None) from the labels by predicted rank; sel picks the rows that are written.
template <bool ALL>
__global__ __launch_bounds__(NDCG_LPW * 64) void ndcg_list_kernel(const float* __restrict__ scores,
                                                                 const float* __restrict__ labels,
                                                                 const int32_t* __restrict__ docids, int64_t n_docs,
                                                                 int B, int L, TopN topn, float* __restrict__ per_list,
                                                                 int32_t* __restrict__ order_out,
                                                                 float* __restrict__ masked_out, NdcgTail tail, MetricSel sel) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sm_s = smem;                 // [LPW][L] ms
  float* sm_y = sm_s + NDCG_LPW * L;  // [LPW][L] my
  float* sm_d = sm_y + NDCG_LPW * L;  // [LPW][L] md
  float* sm_i = sm_d + NDCG_LPW * L;  // [LPW][L] mi
  float* sm_l = sm_i + NDCG_LPW * L;  // ALL: [LPW][L] ml
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * NDCG_LPW + wave;
  const int nch = (L + 63) >> 6;  // 64-document chunks of a list
  unsigned long long* sm_v = reinterpret_cast<unsigned long long*>(sm_l + (ALL ? NDCG_LPW * L : 0));  // ALL: [LPW][nch] mv
  unsigned* arrived = reinterpret_cast<unsigned*>(sm_v + (ALL ? NDCG_LPW * nch : 0));  // waves of this workgroup that finished their list (ultr_ndcg_report)
  if (tail.counter != nullptr) {
    if (threadIdx.x == 0) *arrived = 0u;
    __syncthreads();  // (before the waves without a list leave)
  }
  if (b >= B) return;
  float* ms = sm_s + wave * L;
  float* my = sm_y + wave * L;
  float* md = sm_d + wave * L;
  float* mi = sm_i + wave * L;
  float* ml = sm_l + wave * L;
  unsigned long long* mv = sm_v + wave * nch;
  float mn = INFINITY;
  bool nan_seen = false;
  for (int l = lane; l < L; l += 64) stage_document(scores, labels, docids, n_docs, B, L, b, l, masked_out, ms, my, mn, nan_seen);
  mn = -wave_max(-mn);
  if (__ballot(nan_seen) != 0) mn = __builtin_nanf("");  // torch.min propagates a NaN (fminf drops it)
  for (int l0 = 0; l0 < L; l0 += 64) validate_chunk<ALL>(l0 >> 6, L, lane, mn, ms, my, mv);
  wave_lds_sync();
  const unsigned* mk = reinterpret_cast<const unsigned*>(ms);
  int opa = 0;  // ALL: this lane's correctly ordered pairs
  for (int i = lane; i < L; i += 64) {
    const RankDoc d{i, mk[i], my[i]};
    RankCount n{0, 0, 0};
    unsigned long long vj = 0;
    for (int j = 0; j < L; ++j) {
      if constexpr (ALL) {
        if ((j & 63) == 0) vj = mv[j >> 6];
      }
      count_against<ALL>(n, d, j, mk[j], my[j], vj);
    }
    place_document<ALL>(d, n, mv, ml, md, mi, order_out, b, L, opa);
  }
  wave_lds_sync();
  float whole[ULTR_MAX_METRICS] = {};
  if constexpr (ALL) rank_scans(ml, ms, L, lane, sel.pow_max, (float)opa, whole);  // (the pair count is below 2^24: exact)
  const int width = ALL ? sel.n * topn.n : topn.n;  // floats of a list in per_list, and of the batch means
  cutoff_sums<ALL>(md, mi, ms, L, lane, b, B, topn, sel, whole, per_list, width, tail.counter != nullptr);
  if (tail.counter == nullptr) return;
  // ---- the last workgroup to arrive forms the batch means: every wave waits for its write-through stores to be acknowledged, the
  // workgroup's waves meet (waves without a list left the kernel at its top: the counter counts LISTS, a workgroup adds its own
  // number of them with one relaxed agent-scope increment - 64 increments on one address instead of 256 at config 2) ----------------
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int lists_here = (B - (int)blockIdx.x * NDCG_LPW) < NDCG_LPW ? (B - (int)blockIdx.x * NDCG_LPW) : NDCG_LPW;
  // (the waves of a partial last workgroup that returned early never reach this point: count arrivals instead of a barrier)
  unsigned mine = 0;
  if (lane == 0) mine = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  mine = (unsigned)__builtin_amdgcn_readfirstlane((int)mine);
  if (mine != (unsigned)lists_here - 1u) return;  // not the last wave of this workgroup
  unsigned old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(tail.counter, (unsigned)lists_here, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
  if (old + (unsigned)lists_here != (unsigned)B) return;
  if constexpr (ALL) {
    metrics_means(per_list, B, width, lane, tail);
    return;
  }
  // NDCG alone keeps a tail of its own: its at most 16 means wait in registers and leave together, where metrics_means stores each
  // value before it loads for the next.  Through metrics_means this launch measured about 0.8 us slower on an 8.5 us kernel
  // (profiles/metrics_core.md).  The same sums in the same order; the sequence word is word 16 of this report
  const Src pl = make_src(per_list, (int64_t)B * topn.n);
  float vals[NDCG_MAX_TOPN];
  for (int k = 0; k < topn.n; ++k) {
    float s = 0.f;
    for (int bb = lane; bb < B; bb += 64) s += coh_ld1(pl, (unsigned)(((int64_t)bb * topn.n + k) * 4));  // served from the coherence point
    s = wave_sum(s);
    vals[k] = s / (float)B;
  }
  if (lane == 0) {
    for (int k = 0; k < topn.n; ++k) tail.out[k] = vals[k];
    __hip_atomic_store(tail.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch on this stream
    if (tail.host != nullptr) {
      for (int k = 0; k < topn.n; ++k) __hip_atomic_store(tail.host + k, vals[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(reinterpret_cast<uint32_t*>(tail.host) + NDCG_MAX_TOPN, tail.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---- lists beyond the 64 KiB that four single-wave lists share: ONE workgroup of METRICS_LONG_WAVES waves per list, that list's arrays
// in up to the whole 160 KiB of LDS.  ndcg_list_kernel<true>'s contract and, wherever both take a list, its bits: the row minimum is a
// min (no order), the ranks and the pair count are integers, and every float sum is formed by wave 0 alone, by the functions that
// kernel calls.
#define METRICS_LONG_WAVES 16
#define METRICS_LONG_THREADS (METRICS_LONG_WAVES * 64)
#define METRICS_LDS_MAX (160 * 1024)

// LDS bytes of a workgroup: five [L rounded up to 4] float arrays (the counting loop reads 16 bytes at a time), one validity bit per
// document, and per wave the minimum, the NaN flag and the pair count
static constexpr size_t metrics_long_lds_bytes(int L) {
  return ((size_t)5 * ((L + 3) & ~3) + (size_t)2 * ((L + 63) / 64) + 3 * METRICS_LONG_WAVES) * sizeof(float);
}
// THE length bound of the metric launch (ultr_metrics_max_list): the longest list whose arrays fit 160 KiB
static constexpr int metrics_long_max_list() {
  int L = METRICS_LDS_MAX / (5 * (int)sizeof(float));
  while (metrics_long_lds_bytes(L) > METRICS_LDS_MAX) --L;
  return L;
}
static_assert(metrics_long_max_list() >= 4096, "the long metric kernel takes every list up to 4096 documents");

__global__ __launch_bounds__(METRICS_LONG_THREADS) void metrics_long_kernel(const float* __restrict__ scores, const float* __restrict__ labels,
                                                                            const int32_t* __restrict__ docids, int64_t n_docs, int B, int L,
                                                                            TopN topn, float* __restrict__ per_list,
                                                                            int32_t* __restrict__ order_out, float* __restrict__ masked_out,
                                                                            NdcgTail tail, MetricSel sel) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Lp = (L + 3) & ~3;
  float* ms = smem;     // [Lp] each
  float* my = ms + Lp;
  float* md = my + Lp;
  float* mi = md + Lp;
  float* ml = mi + Lp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int nch = (L + 63) >> 6;
  unsigned long long* mv = reinterpret_cast<unsigned long long*>(ml + Lp);  // [nch]
  float* w_min = reinterpret_cast<float*>(mv + nch);                        // [waves] each wave's minimum
  int* w_nan = reinterpret_cast<int*>(w_min + METRICS_LONG_WAVES);          // [waves] whether it saw a NaN
  int* w_opa = w_nan + METRICS_LONG_WAVES;                                  // [waves] its correctly ordered pairs
  // all waves stride the list; the row minimum and the NaN flag meet in LDS
  float mn = INFINITY;
  bool nan_seen = false;
  for (int l = tid; l < L; l += METRICS_LONG_THREADS) stage_document(scores, labels, docids, n_docs, B, L, b, l, masked_out, ms, my, mn, nan_seen);
  mn = -wave_max(-mn);
  const unsigned long long nan_lanes = __ballot(nan_seen);
  if (lane == 0) {
    w_min[wave] = mn;
    w_nan[wave] = nan_lanes != 0 ? 1 : 0;
  }
  __syncthreads();
  int any_nan = 0;
#pragma unroll
  for (int w = 0; w < METRICS_LONG_WAVES; ++w) {
    mn = fminf(mn, w_min[w]);
    any_nan |= w_nan[w];
  }
  if (any_nan != 0) mn = __builtin_nanf("");  // torch.min propagates a NaN (fminf drops it)
  for (int c = wave; c < nch; c += METRICS_LONG_WAVES) validate_chunk<true>(c, L, lane, mn, ms, my, mv);
  __syncthreads();
  // rank by counting: document i of a thread against every j, four j per 16-byte LDS read (one address per wave: a broadcast)
  const unsigned* mk = reinterpret_cast<const unsigned*>(ms);
  int opa = 0;
  const int L4 = L & ~3;
  for (int i = tid; i < L; i += METRICS_LONG_THREADS) {
    const RankDoc d{i, mk[i], my[i]};
    RankCount n{0, 0, 0};
    unsigned long long vj = 0;
    for (int j = 0; j < L4; j += 4) {
      const uint4 k4 = *reinterpret_cast<const uint4*>(mk + j);
      const float4 y4 = *reinterpret_cast<const float4*>(my + j);
      if ((j & 63) == 0) vj = mv[j >> 6];
      count_against<true>(n, d, j, k4.x, y4.x, vj);
      count_against<true>(n, d, j + 1, k4.y, y4.y, vj);
      count_against<true>(n, d, j + 2, k4.z, y4.z, vj);
      count_against<true>(n, d, j + 3, k4.w, y4.w, vj);
    }
    for (int j = L4; j < L; ++j) {
      if ((j & 63) == 0) vj = mv[j >> 6];
      count_against<true>(n, d, j, mk[j], my[j], vj);
    }
    place_document<true>(d, n, mv, ml, md, mi, order_out, b, L, opa);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) opa += __shfl_xor(opa, d);
  if (lane == 0) w_opa[wave] = opa;
  __syncthreads();  // the last barrier: every wave is still here
  if (wave != 0) return;
  // ---- wave 0 alone: the scans and sums over the ranked arrays ---------------------------------------------------------------------------
  int opa_all = 0;  // an integer up to L * L / 2 < 2^31, converted once
#pragma unroll
  for (int w = 0; w < METRICS_LONG_WAVES; ++w) opa_all += w_opa[w];
  float whole[ULTR_MAX_METRICS] = {};
  rank_scans(ml, ms, L, lane, sel.pow_max, lane == 0 ? (float)opa_all : 0.f, whole);
  const int width = sel.n * topn.n;
  cutoff_sums<true>(md, mi, ms, L, lane, b, B, topn, sel, whole, per_list, width, true);
  // the list that arrives last forms the batch means (no workgroup waits for another)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(tail.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
  if (old + 1u != (unsigned)B) return;
  metrics_means(per_list, B, width, lane, tail);
}

__global__ void ndcg_mean_kernel(const float* __restrict__ per_list, int B, int n_topn, float* __restrict__ out) {
  // mean over the batch, lanes stride the lists, fixed-order wave reduction (one wave per cutoff)
  const int k = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int b = lane; b < B; b += 64) s += per_list[(int64_t)b * n_topn + k];
  s = wave_sum(s);
  if (lane == 0) out[k] = s / (float)B;
}

// the cutoffs of a call as the kernels' argument; false: no list, a count outside 1 .. NDCG_MAX_TOPN, or a cutoff below 1
static bool parse_topn(const int32_t* topn, int32_t n_topn, TopN* t) {
  if (!topn || n_topn <= 0 || n_topn > NDCG_MAX_TOPN) return false;
  t->n = n_topn;
  for (int k = 0; k < n_topn; ++k) {
    if (topn[k] <= 0) return false;
    t->v[k] = topn[k];
  }
  return true;
}

// THE launch of ndcg_list_kernel<false>: per-list values alone (tail.counter == NULL), or with the batch means and the report
static int ndcg_launch(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch, int32_t list_size,
                       const int32_t* topn, int32_t n_topn, int32_t* order_out, float* masked_out, float* ndcg_ws, NdcgTail tail,
                       hipStream_t st) {
  TopN t;
  if (!scores || !labels || !ndcg_ws || batch <= 0 || list_size <= 0 || !parse_topn(topn, n_topn, &t)) return ULTR_E_BADARG;
  const size_t lds = ndcg_lds_bytes(list_size, false);
  if (lds > 64 * 1024) return ULTR_E_UNSUPPORTED;
  UltrProfScope prof(ULTR_K_NDCG, st);
  ULTR_LAUNCH(prof, ndcg_list_kernel<false>, dim3((batch + NDCG_LPW - 1) / NDCG_LPW), dim3(NDCG_LPW * 64), lds, st, scores, labels, docids,
              n_docs, (int)batch, (int)list_size, t, ndcg_ws, order_out, masked_out, tail, MetricSel{});
  return (int)hipGetLastError();
}

extern "C" int ultr_ndcg(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                         int32_t list_size, const int32_t* topn, int32_t n_topn, float* ndcg_out, int32_t* order_out,
                         float* masked_out, float* ndcg_ws, void* stream) {
  if (!ndcg_out) return ULTR_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = ndcg_launch(scores, labels, docids, n_docs, batch, list_size, topn, n_topn, order_out, masked_out, ndcg_ws,
                             NdcgTail{nullptr, nullptr, nullptr, 0u}, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ndcg_mean_kernel, dim3(n_topn), dim3(64), 0, st, (const float*)ndcg_ws, (int)batch, (int)n_topn,
                     ndcg_out);
  return (int)hipGetLastError();
}

// ONE launch: per-list NDCG, batch means by the last wave to finish, optional report into host-mapped memory (include/ultr_hip.h)
extern "C" int ultr_ndcg_report(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                                int32_t list_size, const int32_t* topn, int32_t n_topn, float* ndcg_out, int32_t* order_out,
                                float* masked_out, float* ndcg_ws, uint32_t* counter, float* host_report, uint32_t seq, void* stream) {
  if (!ndcg_out || !counter) return ULTR_E_BADARG;
  return ndcg_launch(scores, labels, docids, n_docs, batch, list_size, topn, n_topn, order_out, masked_out, ndcg_ws,
                     NdcgTail{counter, ndcg_out, host_report, seq}, (hipStream_t)stream);
}

// ONE launch for any of the eight metrics of utils/metrics.py: out [n_metrics][n_topn] in the order of metric_ids (include/ultr_hip.h).
// long_only: metrics_long_kernel at every list size (ultr_metrics_long); otherwise ndcg_list_kernel<true> wherever its LDS fits - the
// routing threshold of ultr_metrics_report - and metrics_long_kernel above
static int metrics_launch(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch, int32_t list_size,
                          const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics, float max_label, float* out,
                          int32_t* order_out, float* masked_out, float* ws, uint32_t* counter, float* host_report, uint32_t seq, void* stream,
                          bool long_only) {
  TopN t;
  if (!scores || !labels || !metric_ids || !out || !ws || !counter || batch <= 0 || list_size <= 0 || n_metrics <= 0 ||
      n_metrics > ULTR_MAX_METRICS || !(fabsf(max_label) < INFINITY) || !parse_topn(topn, n_topn, &t))
    return ULTR_E_BADARG;
  MetricSel sel{};
  sel.n = n_metrics;
  sel.pow_max = exp2f(max_label);
  unsigned seen = 0;
  for (int m = 0; m < n_metrics; ++m) {
    const int id = metric_ids[m];
    if (id < 0 || id >= ULTR_MAX_METRICS || ((seen >> id) & 1u)) return ULTR_E_BADARG;  // unknown or repeated
    seen |= 1u << id;
    sel.id[m] = id;
  }
  // (the per-list block is addressed with 32-bit byte offsets through a buffer descriptor)
  if (list_size > metrics_long_max_list() || (int64_t)batch * n_metrics * n_topn * 4 > INT32_MAX) return ULTR_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const NdcgTail tail{counter, out, host_report, seq};
  const size_t lds = ndcg_lds_bytes(list_size, true);
  if (!long_only && lds <= 64 * 1024) {
    UltrProfScope prof(ULTR_K_NDCG, st);
    ULTR_LAUNCH(prof, ndcg_list_kernel<true>, dim3((batch + NDCG_LPW - 1) / NDCG_LPW), dim3(NDCG_LPW * 64), lds, st, scores, labels, docids,
                n_docs, (int)batch, (int)list_size, t, ws, order_out, masked_out, tail, sel);
    return (int)hipGetLastError();
  }
  const size_t lds_long = metrics_long_lds_bytes(list_size);
  if (lds_long > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(metrics_long_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_long) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  UltrProfScope prof(ULTR_K_NDCG, st);
  ULTR_LAUNCH(prof, metrics_long_kernel, dim3((unsigned)batch), dim3(METRICS_LONG_THREADS), lds_long, st, scores, labels, docids, n_docs,
              (int)batch, (int)list_size, t, ws, order_out, masked_out, tail, sel);
  return (int)hipGetLastError();
}

extern "C" int ultr_metrics_report(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                                   int32_t list_size, const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics,
                                   float max_label, float* out, int32_t* order_out, float* masked_out, float* ws, uint32_t* counter,
                                   float* host_report, uint32_t seq, void* stream) {
  return metrics_launch(scores, labels, docids, n_docs, batch, list_size, topn, n_topn, metric_ids, n_metrics, max_label, out, order_out,
                        masked_out, ws, counter, host_report, seq, stream, false);
}

extern "C" int ultr_metrics_long(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                                 int32_t list_size, const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics,
                                 float max_label, float* out, int32_t* order_out, float* masked_out, float* ws, uint32_t* counter,
                                 float* host_report, uint32_t seq, void* stream) {
  return metrics_launch(scores, labels, docids, n_docs, batch, list_size, topn, n_topn, metric_ids, n_metrics, max_label, out, order_out,
                        masked_out, ws, counter, host_report, seq, stream, true);
}

extern "C" int32_t ultr_metrics_max_list(void) { return metrics_long_max_list(); }
