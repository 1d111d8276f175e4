// ultr_sr_dropout.h - SetRank's dropout (reference SetRank.py:103-117, 141-153: nn.Dropout(rate) behind the embedding FFN, the attention's
// dense layer and the encoder FFN).  Kernels in ultr_sr_dropout.hip, called from ultr_setrank.hip's separate-launch paths.
//
// The mask law: keep(site, t, c) is a pure function of the key and the element - nothing is stored between
// the forward and the backward, the backward draws it again.
//   key      Philox{k0, k1} of (seed, step): k0 = lo32(seed) ^ hi32(step * golden gamma), k1 = hi32(seed) ^ lo32(step)
//   counter  (c0 = t, c1 = (stream << 8) | site, c2 = c >> 2, c3 = SR_DROPOUT_TAG);  the element takes output word c & 3
//            t = l * B + b (position-major token), c = column 0 .. d_model - 1
//   keep     u01(word) >= rate (float32);  y = keep ? v * scale : 0,  scale = 1.0f / (1.0f - rate)
//   site     0: behind input_embedding;  1 + 2 l: behind encoder l's mha.dense;  2 + 2 l: behind encoder l's ffn
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SR_DROPOUT_TAG 0x5352444Fu
#define SR_DROP_ROWS 64  // rows per workgroup (and per column-sum partial) of sr_drop_mask_kernel

struct SrDropArgs {
  uint32_t k0, k1;   // the Philox key of (seed, step)
  uint32_t stream;   // data-parallel rank
  float rate, scale;
  int B, L;          // kernel rows are list-major (n = b L + l); the law counts position-major
};

// ULTR_E_BADARG unless 0 <= rate < 1
int sr_drop_args(float rate, uint64_t seed, uint64_t step, uint32_t stream, int B, int L, SrDropArgs* out);
inline int64_t sr_drop_parts(int64_t T) { return (T + SR_DROP_ROWS - 1) / SR_DROP_ROWS; }

// s = a + D_site(b + bias),  y = LayerNorm(s) gamma + beta;  writes s, mean, rstd, y (b may alias y)
void sr_drop_ln_fwd_launch(const SrDropArgs& a, int site, const float* x, const float* b, const float* bias, int64_t T, int W,
                           const float* gamma, const float* beta, float* sum_out, float* y, float* mean_out, float* rstd_out,
                           hipStream_t st);
// dst = D_site(src) (dst may be src);  part != NULL: part[blk][0 .. W) = column sums of dst over the workgroup's SR_DROP_ROWS rows
void sr_drop_mask_launch(const SrDropArgs& a, int site, const float* src, float* dst, float* part, int64_t T, int W, hipStream_t st);
