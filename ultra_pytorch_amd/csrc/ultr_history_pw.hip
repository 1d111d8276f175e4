// ultr_history_pw.hip - per-click inverse propensity weights of a click model whose examination depends on the click history
// (include/ultr_hip.h: ultr_history_pw; reference OraclePropensityEstimator.getPropensityForOneList on a user-browsing model,
// click_models.py:151-162).
//
// The weight at position l of a list is table[l][last + 1], last = the largest l' < l with a click (-1: none so far).  Nothing here
// depends on a draw, so the previous click is not a serial walk: a ballot of the clicks and the highest set bit below the lane give
// it to every position at once.
//   - list_size <= 32: 64 / W lists per wavefront in segments of W = 8 / 16 / 32 lanes, one lane per position, the ballot cut to the
//     lane's segment (batch 256 x list 10 is 64 wavefronts, not 256);
//   - list_size  > 32: one list per wavefront in chunks of 64 positions, the last click carried wave-uniformly from chunk to chunk.
// Every output is a pure function of its list: no atomics, no dependence on the launch geometry.  pw_out is written in [B, L] order,
// consecutive lanes to consecutive addresses (segments of one wavefront hold consecutive lists).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"

#define HPW_WAVES 4

// rank of the highest set bit of m, or `none` when m == 0
__device__ __forceinline__ int hpw_top_bit(uint64_t m, int none) { return m ? 63 - (int)__builtin_clzll(m) : none; }

template <int W>
__global__ __launch_bounds__(HPW_WAVES * 64) void history_pw_kernel(const float* __restrict__ labels, const float* __restrict__ table,
                                                                   float* __restrict__ pw_out, int B, int L, int all_positions) {
  constexpr int LPV = 64 / W;  // lists per wavefront
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = lane / W, pos = lane % W, base = seg * W;
  const int64_t b = ((int64_t)blockIdx.x * HPW_WAVES + wave) * LPV + seg;
  const bool in = b < B && pos < L;
  const float y = in ? labels[(int64_t)pos * B + b] : 0.f;
  const bool click = in && y > 0.f;
  // every lane of the wavefront takes part in the ballot; the segment's W bits, then the bits below this lane's position
  const uint64_t seg_bits = (__ballot(click) >> base) & ((1ull << W) - 1ull);
  const int last = hpw_top_bit(seg_bits & ((1ull << pos) - 1ull), -1);
  if (in) pw_out[b * L + pos] = (all_positions || click) ? table[(int64_t)pos * L + last + 1] : 0.f;
}

// one list per wavefront, list_size > 32
__global__ __launch_bounds__(HPW_WAVES * 64) void history_pw_long_kernel(const float* __restrict__ labels, const float* __restrict__ table,
                                                                        float* __restrict__ pw_out, int B, int L, int all_positions) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * HPW_WAVES + wave;
  if (b >= B) return;  // wave-uniform: whole wavefronts leave
  int carry = -1;      // the last click of the chunks behind, the same in every lane
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    const bool in = l < L;
    const float y = in ? labels[(int64_t)l * B + b] : 0.f;
    const bool click = in && y > 0.f;
    const uint64_t bits = __ballot(click);
    const int below = hpw_top_bit(bits & ((1ull << lane) - 1ull), -1);
    const int last = below >= 0 ? l0 + below : carry;
    if (in) pw_out[b * L + l] = (all_positions || click) ? table[(int64_t)l * L + last + 1] : 0.f;
    const int top = hpw_top_bit(bits, -1);
    carry = top >= 0 ? l0 + top : carry;
  }
}

extern "C" int ultr_history_pw(const ultr_history_pw_args* a, void* stream) {
  if (!a || !a->labels || !a->table || !a->pw_out || a->batch <= 0 || a->list_size <= 0 ||
      (a->all_positions != 0 && a->all_positions != 1))
    return ULTR_E_BADARG;
  const int B = a->batch, L = a->list_size, all = a->all_positions;
  const int W = L <= 8 ? 8 : (L <= 16 ? 16 : (L <= 32 ? 32 : 0));
  const int64_t per_wg = (int64_t)HPW_WAVES * (W > 0 ? 64 / W : 1);  // lists per workgroup
  const dim3 g((unsigned)((B + per_wg - 1) / per_wg)), blk(HPW_WAVES * 64);
  hipStream_t st = (hipStream_t)stream;
  if (W == 8) hipLaunchKernelGGL(history_pw_kernel<8>, g, blk, 0, st, a->labels, a->table, a->pw_out, B, L, all);
  else if (W == 16) hipLaunchKernelGGL(history_pw_kernel<16>, g, blk, 0, st, a->labels, a->table, a->pw_out, B, L, all);
  else if (W == 32) hipLaunchKernelGGL(history_pw_kernel<32>, g, blk, 0, st, a->labels, a->table, a->pw_out, B, L, all);
  else hipLaunchKernelGGL(history_pw_long_kernel, g, blk, 0, st, a->labels, a->table, a->pw_out, B, L, all);
  return (int)hipGetLastError();
}
