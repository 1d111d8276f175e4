// ultr_rank.h - ranking one list inside one wavefront: the deterministic order key, the Plackett-Luce exponential race and the
// rank by counting.  Shared by online_rerank_kernel (ultr_online.hip) and dbgd_interleave_kernel (ultr_dbgd.hip), so that the online
// feeds and DBGD / MGD rank a list with the same device code.
//
//   keys: deterministic - the score as an unsigned order key (rank_order_key: NaN above +inf, -0 == +0);
//         stochastic    - the exponential race tau (s - max) - log E, E = -log(1 - u) ~ Exp(1): sorting these keys descending draws
//                         a ranking with exactly the Plackett-Luce distribution of sequential sampling without replacement
//                         (np.random.choice(replace=False, p)); a document whose fp32 probability exp(tau (s - max)) / sum is 0
//                         (log p < ln 2^-150) gets key 0, below every drawn one, so those follow in index order (the reference's
//                         `unused` tail);
//   rank by counting over the first len keys (ties by index: stable), as ndcg_list_kernel does.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ultr_device.h"

#define ULTR_RANK_LN_ZERO_PROB -103.97208f  // ln 2^-150: an fp32 probability below it rounds to 0

// the descending order of scores as an unsigned key (ndcg_list_kernel's order): -0 and +0 equal, every NaN equal and above +inf
__device__ __forceinline__ unsigned rank_order_key(float s) {
  if (s != s) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(s == 0.f ? 0.f : s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int wave_max_int(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// all lanes of the wave: LDS writes of this wave before, reads after
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// key[l] for l < len of the scores s[0 .. len) (one list, whole wave).  Stochastic: the race uniform of position l is
// philox_word(c0, c1, l, tag) - the caller's counter words name the list (and ranker) and the stream.
__device__ __forceinline__ void wave_rank_keys(const float* __restrict__ s, int len, bool stochastic, float tau, const Philox& rng,
                                               uint32_t c0, uint32_t c1, uint32_t tag, unsigned* key, int lane) {
  float sum = 0.f, mxs = -INFINITY;
  if (stochastic) {
    for (int l = lane; l < len; l += 64) mxs = fmaxf(mxs, s[l]);
    mxs = wave_max(mxs);
    for (int l = lane; l < len; l += 64) sum += expf(tau * (s[l] - mxs));
    sum = wave_sum(sum);
  }
  for (int l = lane; l < len; l += 64) {
    const float v = s[l];
    unsigned k;
    if (stochastic) {
      const float lw = tau * (v - mxs);
      const float e = -logf(1.0f - u01(philox_word(rng, c0, c1, l, tag)));  // Exp(1); 1 - u is exact for u = k 2^-24
      // fp32 probability 0: exp(lw) / sum rounds to 0 below 2^-150, judged in the log domain (exp in the subnormal range is not
      // reproducible across implementations; log p = lw - log sum is)
      k = (lw - logf(sum) < ULTR_RANK_LN_ZERO_PROB) ? 0u : rank_order_key(lw - logf(e));
    } else {
      k = rank_order_key(v);
    }
    key[l] = k;
  }
  wave_lds_sync();
}

// perm[r] = the index of the r-th largest of key[0 .. len) (ties by index)
template <typename T>
__device__ __forceinline__ void wave_rank_by_count(const unsigned* key, int len, T* perm, int lane) {
  for (int i = lane; i < len; i += 64) {
    const unsigned ki = key[i];
    int r = 0;
    for (int j = 0; j < len; ++j) {
      const unsigned kj = key[j];
      r += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
    }
    perm[r] = (T)i;
  }
}
