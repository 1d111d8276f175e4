// ultr_listloss.h — what the ten list-loss kernels share (ultr_loss.hip, ultr_prs.hip, ultr_pdgd.hip, ultr_twotower.hip,
// ultr_plrank.hip, ultr_affine.hip):
//   * one LDS layout per kernel, a __host__ __device__ struct built from L: the kernel takes its pointers from the offsets, the
//     launcher and ultr_loss_lds_bytes take `bytes` - the two sides cannot drift apart;
//   * launch_list_loss, the one launcher behind the extern "C" entries;
//   * the flat pieces of the pair-walk kernels (pairdebias_kernel, lambdarank_kernel, prs_loss_kernel): indices and slice
//     bounds, staging, rank by counting, the fixed-order fold of the slice partials, the scatter, the workgroup tail store.
// The kernels call the pieces in sequence and keep their own per-pair bodies.
//   * the layouts of the three long-list pair-walk kernels (ultr_loss_long.hip) and loss_route, the host rule that hands a list to them:
//     only a list the short kernel's layout refuses (ultr_step.hip decides with it before the forward is launched).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_plan.h"
#include "ultr_prof.h"

#define LPW ULTR_LOSS_LISTS_PER_WG  // lists per workgroup
#ifndef LOSS_JW
#define LOSS_JW 16  // wavefronts per list of the pair-walk kernels (round 6: 4 -> 16, one list per CU keeps four waves per SIMD busy:
#endif              // pairdebias 7.6 -> 6.2 us, lambdarank 15.3 -> 12.7 us at config 4; tools/ab.sh "--config 4lambda" product jw8 jw16)

#define PDGD_MAX_L 256    // one thread per position in the gradient phase
#define PDGD_THREADS 256
#define PDGD_WAVES (PDGD_THREADS / 64)
__host__ __device__ static inline int pdgd_row(int l) { return l * (l + 3) / 2; }  // row l of the pair weights holds k = 0 .. l+1

#define LOSS_LDS_DEFAULT (64 * 1024)  // dynamic LDS a kernel gets without asking
#define LOSS_LDS_MAX (160 * 1024)     // ... and with hipFuncAttributeMaxDynamicSharedMemorySize: the CU's whole LDS

// ------------------------------------------------------------------------------------------------
// LDS layouts: the float offset of every array of a kernel's dynamic LDS, in allocation order, and the total in bytes
// ------------------------------------------------------------------------------------------------
struct LdsCarve {
  int L;
  int64_t at = 0;
  __host__ __device__ explicit LdsCarve(int L_) : L(L_) {}
  __host__ __device__ int take(int64_t n) {  // n floats, once per workgroup
    const int o = (int)at;
    at += n;
    return o;
  }
  __host__ __device__ int per_list(int64_t n) { return take(LPW * n); }
  __host__ __device__ int64_t end() const { return at * (int64_t)sizeof(float); }
};

struct SoftmaxLds : LdsCarve {  // list_size <= 4095
  static constexpr int64_t limit = LOSS_LDS_DEFAULT;
  int tail = per_list(ultr_tail_len(L));  // [LPW][tail]
  int s = per_list(L);                    // [LPW][L] scores
  int w = per_list(L);                    // [LPW][L] weights
  int64_t bytes = end();
  __host__ __device__ explicit SoftmaxLds(int L_) : LdsCarve(L_) {}
};

// ultr_affine.hip stages what softmax_ce_kernel stages, scores and weights: its layout under the kernel's own name (list_size <= 4095)
using AffineLds = SoftmaxLds;

struct RegemLds : LdsCarve {  // list_size <= 8190
  static constexpr int64_t limit = LOSS_LDS_DEFAULT;
  int tail = per_list(ultr_tail_len(L));  // [LPW][tail]
  int64_t bytes = end();
  __host__ __device__ explicit RegemLds(int L_) : LdsCarve(L_) {}
};

// ultr_twotower.hip keeps nothing but the tail in LDS either: RegressionEM's layout under the kernel's own name (list_size <= 8190)
using TwoTowerLds = RegemLds;

struct DlaLds : LdsCarve {  // list_size <= 3276
  static constexpr int64_t limit = LOSS_LDS_DEFAULT;
  int tail = per_list(ultr_tail_len(L));  // [LPW][tail]
  int s = per_list(L);                    // [LPW][L] scores
  int y = per_list(L);                    // [LPW][L] clicks
  int p = per_list(L);                    // [LPW][L] propensity logits ELU(W_l + b)  (batch independent)
  int64_t bytes = end();
  __host__ __device__ explicit DlaLds(int L_) : LdsCarve(L_) {}
};

struct PairDebiasLds : LdsCarve {  // list_size <= 585
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int tail = per_list(ultr_tail_len(L));          // [LPW][tail]
  int s = per_list(L);                            // [LPW][L] scores
  int c = per_list(L);                            // [LPW][L] clicks
  int rtp = take(L);                              // [L] 1 / t_plus
  int rtm = take(L);                              // [L] 1 / t_minus
  int acc = per_list((int64_t)LOSS_JW * L * 4);   // [LPW][LOSS_JW][L][4]: g, t_plus_loss, t_minus_loss, loss per (slice, position)
  int64_t bytes = end();
  __host__ __device__ explicit PairDebiasLds(int L_) : LdsCarve(L_) {}
};

struct SortedListLds : LdsCarve {  // what lambdarank_kernel and prs_loss_kernel both begin with
  int tail = per_list(ultr_tail_len(L));  // [LPW][tail]
  int s = per_list(L);                    // [LPW][L] raw scores, later d(loss)/d(sorted score)
  int y = per_list(L);                    // [LPW][L] raw labels
  int ps = per_list(L);                   // [LPW][L] scores sorted desc
  int ls = per_list(L);                   // [LPW][L] labels in score order
  int g = per_list(L);                    // [LPW][L] gains 2^l - 1 in score order
  __host__ __device__ explicit SortedListLds(int L_) : LdsCarve(L_) {}
};

struct LambdaRankLds : SortedListLds {  // list_size <= 531
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int tp = take(L);                               // [L] t_plus
  int tm = take(L);                               // [L] t_minus
  int rtp = take(L);                              // [L] 1 / t_plus
  int rtm = take(L);                              // [L] 1 / t_minus
  int d = take(L);                                // [L] discount 1 / log2(rank + 2)
  int pos = per_list(L);                          // [LPW][L] int: sorted position of original index
  int acc = per_list((int64_t)LOSS_JW * L * 4);   // [LPW][LOSS_JW][L][4]: g, t_plus_loss, t_minus_loss, loss
  int64_t bytes = end();
  __host__ __device__ explicit LambdaRankLds(int L_) : SortedListLds(L_) {}
};

struct PrsLds : SortedListLds {  // list_size <= 952
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int ipw = per_list(L);                          // [LPW][L] ipw of the presentation position, in score order
  int pw = per_list(L);                           // [LPW][L] pw = 1 / ipw (0 where ipw == 0), in score order
  int d = take(L);                                // [L] discount 1 / log2(rank + 2)
  int pos = per_list(L);                          // [LPW][L] int: sorted position of original index
  int acc = per_list((int64_t)LOSS_JW * L * 2);   // [LPW][LOSS_JW][L][2]: g, loss
  int64_t bytes = end();
  __host__ __device__ explicit PrsLds(int L_) : SortedListLds(L_) {}
};

struct PdgdLds : LdsCarve {  // list_size <= PDGD_MAX_L (the entry refuses beyond: pdgd_row is 32-bit; 136 KiB there)
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int s = take(L);             // [L] raw scores
  int x = take(L);             // [L] exp of the raw scores (the pair loss)
  int y = take(L);             // [L] labels
  int e = take(L);             // [L] exp-scores
  int D = take(L + 1);         // [L + 1] suffix sums of the exp-scores, D[L] = 0
  int v = take(L);             // [L] int: 1 = a valid document
  int red = take(PDGD_WAVES);  // [PDGD_WAVES]
  int w = take(pdgd_row(L));   // [pdgd_row(L)] pair weights, row l = the clicked document
  int64_t bytes = end();
  __host__ __device__ explicit PdgdLds(int L_) : LdsCarve(L_) {}
};

// ultr_plrank.hip: what a list stages once, and per wave (LOSS_JW waves share a list, each draws its own samples) the race keys, the
// drawn order, the two backward scans and the private partial gradient.  88 L + 37 words: list_size <= 465
struct PlRankLds : LdsCarve {  // list_size <= 465
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int tail = per_list(ultr_tail_len(L));          // [LPW][tail]
  int s = per_list(L);                            // [LPW][L] scores, -inf at a PAD
  int rho = per_list(L);                          // [LPW][L] relevance estimates w gain(y), 0 at a PAD
  int ea = per_list(L);                           // [LPW][L] exp(s - max) scaled, in two factors (ultr_plrank.hip): 0 at a PAD
  int eb = per_list(L);                           // [LPW][L]
  int v = per_list(L);                            // [LPW][L] int: 1 = a valid document
  int hdr = per_list(1);                          // [LPW] int: the list's valid documents
  int d = take(L);                                // [L] discount 1 / log2(rank + 2)
  int red = per_list(LOSS_JW);                    // [LPW][LOSS_JW] each wave's sum of FR_0 over its samples
  int key = per_list((int64_t)LOSS_JW * L);       // [LPW][LOSS_JW][L] unsigned: race keys
  int perm = per_list((int64_t)LOSS_JW * L);      // [LPW][LOSS_JW][L] int: document at each rank
  int z = per_list((int64_t)LOSS_JW * L);         // [LPW][LOSS_JW][L] Z_k
  int fr = per_list((int64_t)LOSS_JW * (L + 1));  // [LPW][LOSS_JW][L + 1] FR_k, FR_L = 0
  int acc = per_list((int64_t)LOSS_JW * L);       // [LPW][LOSS_JW][L] the wave's partial gradient by document
  int64_t bytes = end();
  __host__ __device__ explicit PlRankLds(int L_) : LdsCarve(L_) {}
};

// The long-list kernels (ultr_loss_long.hip): the workgroup's LOSS_LONG_WAVES waves split the OWNED positions, each lane walks every
// partner, so the sums per position stay in registers and no [LOSS_JW][L][NV] array exists: O(L) floats of LDS.  One list per workgroup.
#define LOSS_LONG_WAVES 16
#define LOSS_LONG_THREADS (LOSS_LONG_WAVES * 64)
// A position's sums are formed in two levels, both ascending: LOSS_LONG_CHUNK consecutive partners into a chunk sum, the chunk sums
// into the position's sum - the rounding of an fp32 chain grows with its length: 32 + L / 32 additions deep instead of L.
#define LOSS_LONG_CHUNK 32
static_assert(LPW == 1, "the long-list loss kernels own one list per workgroup: one tail partial per list");

struct PairDebiasLongLds : LdsCarve {  // list_size <= 6823
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int tail = take(ultr_tail_len(L));  // [tail]
  int s = take(L);                    // [L] scores
  int c = take(L);                    // [L] clicks
  int rtp = take(L);                  // [L] 1 / t_plus
  int rtm = take(L);                  // [L] 1 / t_minus
  int red = take(LOSS_LONG_WAVES);    // [LOSS_LONG_WAVES] one partial per wave of a workgroup-wide sum
  int64_t bytes = end();
  __host__ __device__ explicit PairDebiasLongLds(int L_) : LdsCarve(L_) {}
};

struct LambdaRankLongLds : SortedListLds {  // list_size <= 3149
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int tp = take(L);                 // [L] t_plus
  int tm = take(L);                 // [L] t_minus
  int rtp = take(L);                // [L] 1 / t_plus
  int rtm = take(L);                // [L] 1 / t_minus
  int d = take(L);                  // [L] discount 1 / log2(rank + 2)
  int pos = take(L);                // [L] int: sorted position of original index
  int red = take(LOSS_LONG_WAVES);  // [LOSS_LONG_WAVES]
  int64_t bytes = end();
  __host__ __device__ explicit LambdaRankLongLds(int L_) : SortedListLds(L_) {}
};

struct PrsLongLds : SortedListLds {  // list_size <= 3721
  static constexpr int64_t limit = LOSS_LDS_MAX;
  int ipw = take(L);                // [L] ipw of the presentation position, in score order
  int pw = take(L);                 // [L] pw = 1 / ipw (0 where ipw == 0), in score order
  int d = take(L);                  // [L] discount 1 / log2(rank + 2)
  int pos = take(L);                // [L] int: sorted position of original index
  int red = take(LOSS_LONG_WAVES);  // [LOSS_LONG_WAVES]
  int64_t bytes = end();
  __host__ __device__ explicit PrsLongLds(int L_) : SortedListLds(L_) {}
};

// ------------------------------------------------------------------------------------------------
// routing (host): a list the short pair-walk kernel of `algo` takes runs that kernel; only a list it refuses goes to the long one
// ------------------------------------------------------------------------------------------------
enum LossRoute { LOSS_ROUTE_SHORT = 0, LOSS_ROUTE_LONG = 1 };

// dynamic LDS of the long kernel of `algo` at L, ULTR_E_UNSUPPORTED beyond its limit, ULTR_E_BADARG where `algo` has none
static inline int64_t loss_long_bytes(int algo, int L) {
  if (L <= 0) return ULTR_E_BADARG;
  int64_t n;
  switch (algo) {
    case ULTR_ALGO_PAIRDEBIAS: n = PairDebiasLongLds(L).bytes; break;
    case ULTR_ALGO_LAMBDARANK: n = LambdaRankLongLds(L).bytes; break;
    case ULTR_ALGO_PRS: n = PrsLongLds(L).bytes; break;
    default: return ULTR_E_BADARG;
  }
  return n > LOSS_LDS_MAX ? ULTR_E_UNSUPPORTED : n;
}

// "the short layout of `algo` does not fit at L": false for an algorithm without a long kernel (its short entry answers for itself)
static inline bool loss_short_refuses(int algo, int L) {
  if (L <= 0) return false;
  switch (algo) {
    case ULTR_ALGO_PAIRDEBIAS: return PairDebiasLds(L).bytes > PairDebiasLds::limit;
    case ULTR_ALGO_LAMBDARANK: return LambdaRankLds(L).bytes > LambdaRankLds::limit;
    case ULTR_ALGO_PRS: return PrsLds(L).bytes > PrsLds::limit;
    default: return false;
  }
}

// LOSS_ROUTE_SHORT, LOSS_ROUTE_LONG, or ULTR_E_UNSUPPORTED for a list neither kernel takes
static inline int loss_route(int algo, int L) {
  // TwoTower has the one kernel: a list beyond its layout is refused here, before the forward is launched
  if (algo == ULTR_ALGO_TWOTOWER && L > 0 && TwoTowerLds(L).bytes > TwoTowerLds::limit) return ULTR_E_UNSUPPORTED;
  if (algo == ULTR_ALGO_PLRANK && L > 0 && PlRankLds(L).bytes > PlRankLds::limit) return ULTR_E_UNSUPPORTED;  // PLRank likewise
  if (algo == ULTR_ALGO_AFFINE && L > 0 && AffineLds(L).bytes > AffineLds::limit) return ULTR_E_UNSUPPORTED;  // ... and AffineRank
  if (!loss_short_refuses(algo, L)) return LOSS_ROUTE_SHORT;
  return loss_long_bytes(algo, L) >= 0 ? LOSS_ROUTE_LONG : ULTR_E_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// the one launcher: ultr_loss_parts(batch) workgroups of `threads`, under the ULTR_K_LOSS profiling scope
// ------------------------------------------------------------------------------------------------
template <class... KArgs, class... Args>
static int launch_list_loss(void (*kernel)(KArgs...), int threads, int64_t lds_bytes, int64_t lds_limit, int32_t batch, void* stream,
                            Args... args) {
  if (lds_bytes > lds_limit) return ULTR_E_UNSUPPORTED;
  if (lds_bytes > LOSS_LDS_DEFAULT && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  UltrProfScope prof(ULTR_K_LOSS, (hipStream_t)stream);
  ULTR_LAUNCH(prof, kernel, dim3((unsigned)ultr_loss_parts(batch)), dim3(threads), (size_t)lds_bytes, (hipStream_t)stream,
              static_cast<KArgs>(args)...);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// device pieces
// ------------------------------------------------------------------------------------------------
// sum the per-wave tails of a workgroup in fixed order and store the workgroup's partial
__device__ __forceinline__ void store_wg_tail(const float* sm_tail /*[LPW][tail]*/, int tail, float* part) {
  __syncthreads();
  for (int t = threadIdx.x; t < tail; t += blockDim.x) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LPW; ++w) s += sm_tail[w * tail + t];
    part[t] = s;
  }
}

// where a wavefront of a pair-walk kernel stands: LOSS_JW wavefronts share a list, each walks a slice of the partner positions
struct ListWave {
  int lane, wave;
  int lw, jw;  // list of the workgroup, slice of the list
  int b;       // list of the batch
  int lo, hi;  // the slice's partner positions [lo, hi): empty for the last slices of a short list
};
__device__ __forceinline__ ListWave list_wave(int L) {
  ListWave w;
  w.lane = threadIdx.x & 63, w.wave = threadIdx.x >> 6;
  w.lw = w.wave / LOSS_JW, w.jw = w.wave - w.lw * LOSS_JW;
  w.b = blockIdx.x * LPW + w.lw;
  const int len = (L + LOSS_JW - 1) / LOSS_JW;
  w.lo = w.jw * len, w.hi = (w.lo + len < L) ? w.lo + len : L;
  return w;
}

// wave 0 of a list zeroes the list's tail and stages its raw scores [B, L] and labels [L, B]
__device__ __forceinline__ void stage_list(const ListWave& w, const float* __restrict__ scores, const float* __restrict__ labels, int B,
                                           int L, int tail, float* mt, float* ms, float* my) {
  if (w.jw == 0) {
    for (int t = w.lane; t < tail; t += 64) mt[t] = 0.f;
    if (w.b < B)
      for (int l = w.lane; l < L; l += 64) {
        ms[l] = scores[(int64_t)w.b * L + l];
        my[l] = labels[(int64_t)l * B + w.b];
      }
  }
}

// Rank by counting, stable (ties broken by original index): position i's rank rs among the scores and ry among the labels, L
// compares each from LDS; with its gain 2^y - 1 and its term of the ideal DCG
struct Ranked {
  float s, y;  // the position's own score and label
  int rs, ry;
  float gain, idcg;
};
__device__ __forceinline__ Ranked rank_by_counting(const float* ms, const float* my, int L, int i) {
  const float si = ms[i], yi = my[i];
  int rs = 0, ry = 0;
  for (int j = 0; j < L; ++j) {
    const float sj = ms[j], yj = my[j];
    rs += (sj > si || (sj == si && j < i)) ? 1 : 0;
    ry += (yj > yi || (yj == yi && j < i)) ? 1 : 0;
  }
  // dcg(): sum (2^l - 1) / ln(rank + 1), rank 1-based -> ln(ry + 2)   (lambda_rank.py:262-266, prs_rank.py:207-226)
  return Ranked{si, yi, rs, ry, exp2f(yi) - 1.0f, (exp2f(yi) - 1.0f) / logf((float)ry + 2.0f)};
}

// the NV partial sums of (list lw, slice jw, position i) in sm_acc [LPW][LOSS_JW][L][NV]
template <int NV>
__device__ __forceinline__ float* slice_acc(float* sm_acc, int lw, int jw, int L, int i) {
  return sm_acc + ((size_t)(lw * LOSS_JW + jw) * L + i) * NV;
}

// v[k] = position i's k-th partial summed over the slices in the order 0, 1, ..., LOSS_JW - 1
template <int NV>
__device__ __forceinline__ void fold_slices(float* sm_acc, int lw, int L, int i, float (&v)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float t = slice_acc<NV>(sm_acc, lw, 0, L, i)[k];
#pragma unroll
    for (int w = 1; w < LOSS_JW; ++w) t += slice_acc<NV>(sm_acc, lw, w, L, i)[k];
    v[k] = t;
  }
}

// gradients by sorted position (ms[], written by the lane of the sorted position) to presentation order: read by the lane owning
// the original index
__device__ __forceinline__ void scatter_sorted(const ListWave& w, int B, int L, const float* ms, const int* pos,
                                               float* __restrict__ dscores) {
  __syncthreads();
  if (w.b < B && w.jw == 0)
    for (int i = w.lane; i < L; i += 64) dscores[(int64_t)w.b * L + i] = ms[pos[i]];
}
