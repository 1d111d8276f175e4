// ultr_sr_attn.h - SetRank's self-attention launches (kernels in ultr_sr_attn.hip and, for lists beyond the one-pass kernels' bounds, the
// streaming kernels of ultr_sr_attn_long.hip; called from ultr_setrank_forward / _backward).
// No projections: q = k = v = x[:, head slice] (SetRank.py:33-37, 54-66, 159-195).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"

struct SrAttnShape {
  int d, dh, H;   // d_model, head depth, heads
  int att_f16;    // ultr_setrank_desc.attention_dtype == ULTR_ATTN_FP16
  int long_min;   // ULTR_SR_ATTN_LONG_MIN: the forward streams the keys from this list size on (always beyond SR_ATTN_ONE_PASS_MAX)
  int stream_bwd; // ultr_setrank_desc.flags & ULTR_MODEL_SR_STREAM_BWD: the backward streams where the one-pass backward refuses (and
                  // from long_min on), and the forward streams at the same list sizes (the streaming backward reads the forward's lse)
};
constexpr int SR_ATTN_ONE_PASS_MAX = 256;  // the longest list of the one-pass kernels (ultr_sr_attn.hip: 64 lanes x SR_KPL keys)

// the matrix-core kernels take this shape (list_size <= 128, head depth 16 / 32 / 64, 16-byte aligned head slices); else the scalar kernels
bool sr_attn_mfma_ok(const SrAttnShape& s, int L);
// THE dispatch: the kernel family (ultr_setrank_attn_path_id, include/ultr_hip.h) the forward (backward = 0) / the backward (backward = 1)
// takes at this list size, or ULTR_E_UNSUPPORTED.  sr_attn_supported, sr_attn_forward and sr_attn_backward all go through it, so a shape the
// gate admits is a shape the launch takes.  split_half: the caller's knobs allow the split-half backward kernel (read by the backward only)
int sr_attn_path(const SrAttnShape& s, int L, int backward, bool split_half);
// 0 or ULTR_E_UNSUPPORTED: can the forward (backward = 0) / the backward (backward = 1) run at this list size
int sr_attn_supported(const SrAttnShape& s, int L, int backward);
// A[T, d] = softmax(x x^T / sqrt(dh)) x per (list, head), lse[T, H] the row statistic the backward reads
int sr_attn_forward(const SrAttnShape& s, const float* x, int batch, int L, float* A, float* lse, hipStream_t st);
// dx += the attention path's gradient; split_half: the caller's knobs (ULTR_SR_ATTN_H3 and its per-layer mask) allow the split-half kernel.
// tws: [T, H] floats of the caller's workspace for t = dA . A, read and written by the streaming kernels only (s.stream_bwd; else unused)
int sr_attn_backward(const SrAttnShape& s, bool split_half, const float* x, const float* dA, const float* Aout, const float* lse, int batch, int L,
                     float* dx, float* tws, hipStream_t st);
// the same forward with the keys streamed through LDS in tiles (ultr_sr_attn_long.hip): any list size.  mfma: head depth 16 / 32 / 64
// with 16-byte aligned head slices on the fp32 matrix cores; otherwise the scalar kernel, any head depth
int sr_attn_forward_long(const SrAttnShape& s, bool mfma, const float* x, int batch, int L, float* A, float* lse, hipStream_t st);
// the scalar streaming kernel's LDS request, a function of the head depth alone, fits a CU (head depth up to about 420)
bool sr_attn_long_scalar_fits(int dh);
// the streaming BACKWARD (ultr_sr_attn_long.hip): a pre-pass writes t = dA . A per (token, head) to tws [T, H], then every workgroup owns a
// block of tokens of one (list, head) in both roles, query and key, walks the list in partner tiles and writes its own rows of dx.
// lse is the forward's row statistic (any forward kernel that writes one).  mfma as for the forward
int sr_attn_backward_long(const SrAttnShape& s, bool mfma, const float* x, const float* dA, const float* Aout, const float* lse, int batch, int L,
                          float* dx, float* tws, hipStream_t st);
// ... and its scalar kernel's LDS request fits a CU (head depth up to about 250)
bool sr_attn_bwd_long_scalar_fits(int dh);

// a launch's dynamic LDS request: beyond 64 KiB the kernel has to be told; beyond a CU's 160 KiB the shape is refused
template <typename K>
inline int set_dyn_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return ULTR_E_UNSUPPORTED;
  if (bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return ULTR_E_UNSUPPORTED;
  return 0;
}

// tile  D[row = 16 ta + (4 q + r)][col = block of bf] = sum_k  a[16 ta + i][k] * bf[i][k]   (a from LDS, bf = fragments)
template <int DH>
__device__ __forceinline__ f32x4 sr_tile_nt(const float* arow, const float4 (&bf)[DH / 16]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int f = 0; f < DH / 16; ++f) {
    const float4 a4 = ld4(arow + 4 * f);
    acc = mfma16(a4.x, bf[f].x, acc);
    acc = mfma16(a4.y, bf[f].y, acc);
    acc = mfma16(a4.z, bf[f].z, acc);
    acc = mfma16(a4.w, bf[f].w, acc);
  }
  return acc;
}
