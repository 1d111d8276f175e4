// ultr_propensity.hip - the randomized click experiment behind an inverse-propensity table (include/ultr_hip.h:
// ultr_propensity_count; reference RandomizedPropensityEstimator.estimateParametersFromModel, propensity_estimator.py:95-118).
//
// A session is tiny (pick a list, shuffle its n labels, n click decisions, a handful of clicks) and every click lands on one of
// about lmax^2 / 2 counters, so the launch is built around the histogram:
//   - persistent workgroups (4 waves) loop over the sessions and count in a per-workgroup LDS histogram of 32-bit words, stored as
//     the lower triangle (row n - 1 holds positions 0 .. n - 1): 33 KB at lmax = 128, 220 bytes at lmax = 10;
//   - one flush per workgroup at the end, 64-bit integer atomic adds of the non-zero words: integer sums do not depend on the
//     order or on the grid, so the table is bit-reproducible (same-word global atomics serialise at roughly 88 per us - adding every
//     click to global memory directly would be the whole run time);
//   - lmax <= 32: a wavefront runs 64 / W sessions at once in segments of W = 8 / 16 / 32 lanes (one lane per position, all per-lane
//     arithmetic; the cascade's first click is a ballot cut to the segment, the user-browsing walk steps all segments together);
//     lmax > 32: one session per wavefront through wave_click_walk (ultr_click.h), as click_draw does.
// Which wave or segment runs session s does not enter the draw: counters are (lo32(s), hi32(s), group, tag) under click_draw's key
// with step = 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_click.h"
#include "ultr_device.h"
#include "ultr_feed.h"
#include "ultr_rank.h"

#define PROP_WAVES 4
#define PROP_MAX_GRID 1024            // 256 CUs x 4 workgroups: every SIMD holds a wave even at the largest histogram
#define PROP_MIN_TRIPS 16             // sessions per wave slot below which more workgroups only add flush atomics
#define PROP_MAX_LAUNCH_SESSIONS ((int64_t)1 << 31)  // a workgroup's share stays below 2^32: its 32-bit words cannot wrap

struct PropSession {
  int64_t q;
  int n;
};

// the list of session s: (q, n = lengths[q] clamped to [0, lmax]); n = 0 for a session outside the call's range
__device__ __forceinline__ PropSession prop_pick(const ultr_propensity_args& a, const Philox& rng, uint64_t s, bool active) {
  uint32_t c[4] = {(uint32_t)s, (uint32_t)(s >> 32), 0xFFFFFFFFu, ULTR_QUERY_TAG};
  rng(c);
  PropSession p;
  p.q = (int64_t)((double)u01(c[0]) * (double)a.n_queries);
  if (p.q >= a.n_queries) p.q = a.n_queries - 1;
  const int n = active ? a.lengths[p.q] : 0;
  p.n = n < 0 ? 0 : (n > a.lmax ? a.lmax : n);
  return p;
}

// 64 / W sessions per wavefront trip, lmax <= W <= 32
template <int W>
__device__ __forceinline__ void prop_packed(const ultr_propensity_args& a, const Philox& rng, unsigned* hist, unsigned* key, int* perm) {
  constexpr int SPW = 64 / W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, seg = lane / W, pos = lane % W, base = seg * W;
  const ClickModel cm = click_model_of(a);
  ClickModel each = cm;  // the decision of each position on its own: the cascade's cut and the user-browsing walk run per segment below
  each.model = cm.model == ULTR_CLICK_TRUST ? ULTR_CLICK_TRUST : ULTR_CLICK_PBM;  // (trust bias carries no state either)
  const uint64_t stride = (uint64_t)gridDim.x * PROP_WAVES * SPW;
  const uint64_t slot = ((uint64_t)blockIdx.x * PROP_WAVES + wave) * SPW + seg;
  const int64_t trips = (a.n_sessions + (int64_t)stride - 1) / (int64_t)stride;
  for (int64_t t = 0; t < trips; ++t) {
    const uint64_t k = (uint64_t)t * stride + slot;
    const bool active = k < (uint64_t)a.n_sessions;
    const uint64_t s = a.first_session + k;
    const PropSession p = prop_pick(a, rng, s, active);
    const int n = p.n;
    const bool in = pos < n;
    if (in) key[lane] = philox_word(rng, (uint32_t)s, (uint32_t)(s >> 32), pos, ULTR_SHUFFLE_TAG);
    wave_lds_sync();
    wave_rank_by_count(key + base, n, perm + base, pos);
    wave_lds_sync();
    float y = 0.f, u = 0.f;
    if (in) {
      y = a.labels[p.q * a.lmax + perm[lane]];
      u = u01(philox_word(rng, (uint32_t)s, (uint32_t)(s >> 32), pos, ULTR_CLICK_TAG));
    }
    float ck;
    if (cm.model == ULTR_CLICK_UBM) {
      // click_decide's walk with a `last click` per segment: every lane follows its own segment's list
      const float ratio = in ? u / click_prob_of(cm, y) : 0.f;
      int last = -1;
      ck = 0.f;
      for (int r = 0; r < W; ++r) {
        const float rk = __shfl(ratio, base + r);
        if (r < n) {
          const bool hit = rk < ubm_exam_prob(cm, r, r - last);
          if (hit) last = r;
          if (hit && pos == r) ck = 1.f;
        }
      }
    } else {
      bool cb = false;
      int lc = -1;
      ck = click_decide(each, n, 0, pos, in, y, u, cb, lc);
      if (cm.model == ULTR_CLICK_CASCADE) {  // only the first click of the list counts: the ballot of click_decide, cut to the segment
        const uint64_t hit = (__ballot(ck > 0.f) >> base) & ((1ull << W) - 1ull);
        const int first = hit ? (int)__builtin_ctzll(hit) : W;
        if (pos > first) ck = 0.f;
      }
    }
    if (ck > 0.f) atomicAdd(&hist[(n - 1) * n / 2 + pos], 1u);
    // the next trip's keys and ranks go to the same LDS words: this trip's reads of them are done (the label gather above is
    // consumed by the decision, which every lane has passed by the time it reaches the next wave_lds_sync)
  }
}

// one session per wavefront trip, lmax <= 128
__device__ __forceinline__ void prop_wave(const ultr_propensity_args& a, const Philox& rng, unsigned* hist, unsigned* key, int* perm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ClickModel cm = click_model_of(a);
  const uint64_t stride = (uint64_t)gridDim.x * PROP_WAVES;
  const uint64_t slot = (uint64_t)blockIdx.x * PROP_WAVES + wave;
  for (uint64_t k = slot; k < (uint64_t)a.n_sessions; k += stride) {
    const uint64_t s = a.first_session + k;
    const uint32_t c0 = (uint32_t)s, c1 = (uint32_t)(s >> 32);
    const PropSession p = prop_pick(a, rng, s, true);
    const int n = __builtin_amdgcn_readfirstlane(p.n);
    for (int l = lane; l < n; l += 64) key[l] = philox_word(rng, c0, c1, l, ULTR_SHUFFLE_TAG);
    wave_lds_sync();
    wave_rank_by_count(key, n, perm, lane);
    wave_lds_sync();
    wave_click_walk(
        cm, rng, c0, c1, ULTR_CLICK_TAG, n, lane, [&](int l) { return a.labels[p.q * a.lmax + perm[l]]; },
        [&](int l, float ck) {
          if (ck > 0.f) atomicAdd(&hist[(n - 1) * n / 2 + l], 1u);
        });
    wave_lds_sync();  // perm is read above and rewritten by the next session
  }
}

// dynamic LDS: hist [lmax (lmax + 1) / 2] | key [4 waves][KN] | perm [4 waves][KN], KN = 64 (packed) or ULTR_PROPENSITY_MAX_L
template <int W>
__global__ __launch_bounds__(PROP_WAVES * 64) void propensity_count_kernel(ultr_propensity_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned prop_lds[];
  constexpr int KN = W > 0 ? 64 : ULTR_PROPENSITY_MAX_L;
  const int lmax = a.lmax, tri = lmax * (lmax + 1) / 2, wave = threadIdx.x >> 6;
  unsigned* hist = prop_lds;
  unsigned* key = prop_lds + tri + wave * KN;
  int* perm = reinterpret_cast<int*>(prop_lds + tri + PROP_WAVES * KN) + wave * KN;
  for (int i = threadIdx.x; i < tri; i += PROP_WAVES * 64) hist[i] = 0u;
  __syncthreads();
  const Philox rng{(uint32_t)a.seed, (uint32_t)(a.seed >> 32)};  // click_draw's key with step = 0
  if constexpr (W > 0) prop_packed<W>(a, rng, hist, key, perm);
  else prop_wave(a, rng, hist, key, perm);
  __syncthreads();
  for (int row = 0; row < lmax; ++row)
    for (int r = threadIdx.x; r <= row; r += PROP_WAVES * 64) {
      const unsigned v = hist[row * (row + 1) / 2 + r];
      if (v != 0u) atomicAdd(a.click_count + (int64_t)row * lmax + r, (unsigned long long)v);
    }
}

static bool propensity_args_ok(const ultr_propensity_args* a) {
  return a && a->labels && a->lengths && a->click_count && a->n_queries > 0 && a->lmax > 0 && a->n_sessions >= 0 &&
         click_model_ok(click_model_of(*a));
}

extern "C" int ultr_propensity_count(const ultr_propensity_args* a, void* stream) {
  if (!propensity_args_ok(a)) return ULTR_E_BADARG;
  if (a->lmax > ULTR_PROPENSITY_MAX_L) return ULTR_E_UNSUPPORTED;
  const int lmax = a->lmax;
  const int W = lmax <= 8 ? 8 : (lmax <= 16 ? 16 : (lmax <= 32 ? 32 : 0));
  const int64_t per_trip = PROP_WAVES * (W > 0 ? 64 / W : 1);  // sessions a workgroup runs per trip
  const size_t lds = sizeof(unsigned) * ((size_t)lmax * (lmax + 1) / 2 + 2 * PROP_WAVES * (W > 0 ? 64 : ULTR_PROPENSITY_MAX_L));
  ultr_propensity_args c = *a;
  for (int64_t done = 0; done < a->n_sessions; done += PROP_MAX_LAUNCH_SESSIONS) {
    c.first_session = a->first_session + (uint64_t)done;
    c.n_sessions = a->n_sessions - done < PROP_MAX_LAUNCH_SESSIONS ? a->n_sessions - done : PROP_MAX_LAUNCH_SESSIONS;
    int64_t grid = (c.n_sessions + per_trip * PROP_MIN_TRIPS - 1) / (per_trip * PROP_MIN_TRIPS);
    grid = grid < 1 ? 1 : (grid > PROP_MAX_GRID ? PROP_MAX_GRID : grid);
    const dim3 g((unsigned)grid), b(PROP_WAVES * 64);
    if (W == 8) hipLaunchKernelGGL(propensity_count_kernel<8>, g, b, lds, (hipStream_t)stream, c);
    else if (W == 16) hipLaunchKernelGGL(propensity_count_kernel<16>, g, b, lds, (hipStream_t)stream, c);
    else if (W == 32) hipLaunchKernelGGL(propensity_count_kernel<32>, g, b, lds, (hipStream_t)stream, c);
    else hipLaunchKernelGGL(propensity_count_kernel<0>, g, b, lds, (hipStream_t)stream, c);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return 0;
}
