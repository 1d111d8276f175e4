// ultr_gsf.hip - the GSF ranking model (include/ultr_hip.h: ultr_gsf_*): the DNN's layers on groups of m documents, the circular windows
// of the (shuffled) list, each group's m outputs summed back into document scores.  Geometry and buffer layouts: ultr_gsf_plan.h;
// DESIGN.md section 3e.  Row r = b L + g is group g of list b; slot j of it holds the document at place (g + j) mod L.
//
//   forward   gsf_stats0_kernel (the statistics of the m gathered rows side by side; the table of each row's m documents) -> layer 0 on
//             ugemm::run with the gathering producer AGroupLN -> per hidden layer gsf_rowstats_kernel + ugemm::run (ALayerNorm) ->
//             gsf_head_fwd_kernel (LayerNorm + m dot products per row; no hidden layer: a ugemm::run of m columns) -> gsf_fold_kernel
//   backward  gsf_head_bwd_kernel (d o by the gather law, d u of the head) -> per layer, head first: RgCsTable (bias, beta, gamma
//             partials per row chunk), rg_wgrad (the rows split over the grid; both in ultr_rowgrad.hip), gsf_ln_bwd_kernel (LayerNorm backward x act'),
//             ugemm::run (data gradient) -> ONE fold launch (every partial, the loss partials of the step tail)
//
// LDS: ugemm's tiles (forward products 60 KiB / 40 KiB per workgroup at more than / up to 64 outputs, data gradients 52 / 36 KiB), the
// 2 KiB combine of rg_colsum_kernel, nothing else; no atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_gemm.h"
#include "ultr_gsf_plan.h"
#include "ultr_plan.h"
#include "ultr_rowgrad.h"

namespace {

// ---- the training shuffle: one thread per list, Fisher-Yates from the identity ----------------------------------------------------------
__global__ __launch_bounds__(64) void gsf_shuffle_kernel(uint64_t seed, uint64_t step, int B, int L, int32_t* __restrict__ perm) {
  const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= B) return;
  const Philox rng = philox_step_key(seed, step);
  int32_t* p = perm + (int64_t)b * L;
  for (int l = 0; l < L; ++l) p[l] = l;
  for (int i = L - 1; i >= 1; --i) {
    const uint32_t r = philox_word(rng, (uint32_t)b, 0u, i, ULTR_GSF_SHUFFLE_TAG);
    const int j = (int)(((uint64_t)r * (uint64_t)(i + 1)) >> 32);
    const int32_t t = p[i];
    p[i] = p[j];
    p[j] = t;
  }
}

// the document at place `place` of list b, or -1: a PAD, or an entry of perm outside the list (nothing is read through such an entry)
__device__ __forceinline__ int gsf_doc_at(const int32_t* __restrict__ docids, const int32_t* __restrict__ perm, int64_t n_docs, int B, int L,
                                          int b, int place) {
  int pos = place;
  if (perm != nullptr) pos = perm[(int64_t)b * L + place];
  if (pos < 0 || pos >= L) return -1;
  const int id = docids[(int64_t)pos * B + b];
  return (id >= 0 && id < n_docs) ? id : -1;
}

// ---- statistics of a group's m rows side by side (one wave per group, two passes; a PAD is the zero row) --------------------------------
// also writes slots[r][j] = the byte offset of slot j's feature row (ULTR_OOB: a PAD, or j >= m): the table AGroupLN gathers through
__global__ __launch_bounds__(256) void gsf_stats0_kernel(const float* __restrict__ feats, const int32_t* __restrict__ docids,
                                                         const int32_t* __restrict__ perm, int64_t n_docs, int B, int L, int64_t T, int F, int m,
                                                         uint32_t* __restrict__ slots, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                         float* __restrict__ xhat /* NULL: scoring */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= T) return;
  const int b = (int)((uint32_t)r / (uint32_t)L), g = (int)((uint32_t)r % (uint32_t)L);
  const float* row[GSF_MAX_GROUP];
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j) {
    row[j] = nullptr;
    if (j < m) {
      const int id = gsf_doc_at(docids, perm, n_docs, B, L, b, (g + j) % L);
      if (id >= 0) row[j] = feats + (int64_t)id * F;
    }
    if (lane == j) slots[r * GSF_MAX_GROUP + j] = row[j] != nullptr ? (uint32_t)((row[j] - feats) * 4) : ULTR_OOB;
  }
  const float n = (float)m * (float)F;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j)
    if (j < m && row[j] != nullptr)
      for (int c = lane * 4; c < F; c += 256) {
        const float4 v = ld4(row[j] + c);
        s += (v.x + v.y) + (v.z + v.w);
      }
  const float mean = wave_sum(s) / n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j)
    if (j < m)
      for (int c = lane * 4; c < F; c += 256) {
        const float4 v = row[j] != nullptr ? ld4(row[j] + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / n + ULTR_LN_EPS);
  if (xhat != nullptr) {
    float* xr = xhat + r * ((int64_t)m * F);
#pragma unroll
    for (int j = 0; j < GSF_MAX_GROUP; ++j)
      if (j < m)
        for (int c = lane * 4; c < F; c += 256) {
          const float4 v = row[j] != nullptr ? ld4(row[j] + c) : make_float4(0.f, 0.f, 0.f, 0.f);
          st4(xr + j * F + c, make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd));
        }
  }
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// ---- statistics of consecutive rows (one wave per row, two passes) -----------------------------------------------------------------------
__device__ __forceinline__ void gsf_row_stats(const float* __restrict__ xr, int K, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = lane * 4; c < K; c += 256) {
    const float4 v = ld4(xr + c);
    s += (v.x + v.y) + (v.z + v.w);
  }
  mean = wave_sum(s) / (float)K;
  float q = 0.f;
  for (int c = lane * 4; c < K; c += 256) {
    const float4 v = ld4(xr + c);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + ULTR_LN_EPS);
}
__global__ __launch_bounds__(256) void gsf_rowstats_kernel(const float* __restrict__ x, int64_t T, int K, float* __restrict__ mean_out,
                                                           float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= T) return;
  float mean, rstd;
  gsf_row_stats(x + r * K, K, lane, mean, rstd);
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// ---- the head: o[r][j] = LayerNorm(x[r]) . W[j] + bias[j], j < m (one wave per row) ------------------------------------------------------
// m <= 8 columns: a matrix-core tile would multiply 16 x 64 outputs to keep at most 8 and wants a statistics pass in front; here the row
// is read once from HBM (its two further passes hit L1), W (m K floats) stays in L1 and the sums are one fixed DPP tree per column.
__global__ __launch_bounds__(256) void gsf_head_fwd_kernel(const float* __restrict__ x, int64_t T, int K, int m, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ mean_out,
                                                           float* __restrict__ rstd_out, float* __restrict__ o) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= T) return;
  const float* xr = x + r * K;
  float mean, rstd;
  gsf_row_stats(xr, K, lane, mean, rstd);
  float acc[GSF_MAX_GROUP];
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j) acc[j] = 0.f;
  for (int c = lane * 4; c < K; c += 256) {
    const float4 v = ld4(xr + c), ga = ld4(gamma + c), be = ld4(beta + c);
    const float ux = (v.x - mean) * rstd * ga.x + be.x, uy = (v.y - mean) * rstd * ga.y + be.y;
    const float uz = (v.z - mean) * rstd * ga.z + be.z, uw = (v.w - mean) * rstd * ga.w + be.w;
#pragma unroll
    for (int j = 0; j < GSF_MAX_GROUP; ++j)
      if (j < m) {
        const float4 w = ld4(W + (int64_t)j * K + c);
        acc[j] = fmaf(uw, w.w, fmaf(uz, w.z, fmaf(uy, w.y, fmaf(ux, w.x, acc[j]))));
      }
  }
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j)
    if (j < m) {
      const float t = wave_sum(acc[j]);
      if (lane == 0) o[r * m + j] = t + bias[j];
    }
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// ---- the fold: score[perm[p]] = sum_j o[(p - j) mod L][j], j = 0 .. m - 1 in that order (one thread per place) ---------------------------
__global__ __launch_bounds__(256) void gsf_fold_kernel(const float* __restrict__ o, const int32_t* __restrict__ perm, int L, int64_t T, int m,
                                                       float* __restrict__ scores) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int b = (int)((uint32_t)t / (uint32_t)L), p = (int)((uint32_t)t % (uint32_t)L);
  const int dst = perm != nullptr ? perm[t] : p;
  if (dst < 0 || dst >= L) return;
  float s = 0.f;
  for (int j = 0; j < m; ++j) {
    const int g = (p + L - j % L) % L;
    s += o[((int64_t)b * L + g) * m + j];
  }
  scores[(int64_t)b * L + dst] = s;
}

// ---- backward of the fold and of the head's product (one wave per row) -------------------------------------------------------------------
// d o[r][j] = dscores[perm[(g + j) mod L]] (an entry of perm outside the list: 0);  d u[r][c] = sum_j d o[r][j] W[j][c]
__global__ __launch_bounds__(256) void gsf_head_bwd_kernel(const float* __restrict__ dscores, const int32_t* __restrict__ perm, int L, int64_t T,
                                                           int m, int K, const float* __restrict__ W, float* __restrict__ dout,
                                                           float* __restrict__ du) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= T) return;
  const int b = (int)((uint32_t)r / (uint32_t)L), g = (int)((uint32_t)r % (uint32_t)L);
  float d[GSF_MAX_GROUP];
#pragma unroll
  for (int j = 0; j < GSF_MAX_GROUP; ++j) {
    d[j] = 0.f;
    if (j < m) {
      const int place = (g + j) % L;
      const int pos = perm != nullptr ? perm[(int64_t)b * L + place] : place;
      if (pos >= 0 && pos < L) d[j] = dscores[(int64_t)b * L + pos];
      if (lane == j) dout[r * m + j] = d[j];
    }
  }
  for (int c = lane * 4; c < K; c += 256) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < GSF_MAX_GROUP; ++j)
      if (j < m) {
        const float4 w = ld4(W + (int64_t)j * K + c);
        a.x = fmaf(d[j], w.x, a.x); a.y = fmaf(d[j], w.y, a.y); a.z = fmaf(d[j], w.z, a.z); a.w = fmaf(d[j], w.w, a.w);
      }
    st4(du + r * K + c, a);
  }
}

// ---- LayerNorm backward and the activation derivative below it (one wave per row) --------------------------------------------------------
// x = the layer's input = act(z) of the layer below; dz = rstd (dxh - mean(dxh) - xh mean(dxh xh)) act'(z), dxh = du gamma
__global__ __launch_bounds__(256) void gsf_ln_bwd_kernel(const float* __restrict__ du, const float* __restrict__ x, const float* __restrict__ mean_in,
                                                         const float* __restrict__ rstd_in, const float* __restrict__ gamma, int64_t T, int K,
                                                         int act, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= T) return;
  const float* xr = x + r * K;
  const float* dr = du + r * K;
  const float mean = mean_in[r], rstd = rstd_in[r];
  float s[2] = {0.f, 0.f};
  for (int c = lane * 4; c < K; c += 256) {
    const float4 v = ld4(xr + c), d = ld4(dr + c), ga = ld4(gamma + c);
    const float hx = (v.x - mean) * rstd, hy = (v.y - mean) * rstd, hz = (v.z - mean) * rstd, hw = (v.w - mean) * rstd;
    const float ex = d.x * ga.x, ey = d.y * ga.y, ez = d.z * ga.z, ew = d.w * ga.w;
    s[0] += (ex + ey) + (ez + ew);
    s[1] += (ex * hx + ey * hy) + (ez * hz + ew * hw);
  }
  wave_sum_n<2>(s);
  const float m1 = s[0] / (float)K, m2 = s[1] / (float)K;
  for (int c = lane * 4; c < K; c += 256) {
    const float4 v = ld4(xr + c), d = ld4(dr + c), ga = ld4(gamma + c);
    const float in[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d.x, d.y, d.z, d.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w};
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (in[e] - mean) * rstd;
      out[e] = rstd * (dd[e] * gg[e] - m1 - xh * m2) * act_grad_from_out(in[e], act);
    }
    st4(dz + r * K + c, make_float4(out[0], out[1], out[2], out[3]));
  }
}

// ---- the A operand of the first product ----------------------------------------------------------------------------------------------------
// Row r = b L + g, contraction index k in slot k / F: the feature row of the document at place (g + k / F) mod L (a PAD is the zero row),
// LayerNorm applied from the row's statistics: (x - mean[r]) rstd[r] gamma[k] + beta[k].  F is a multiple of 4, so a 16-byte piece never
// straddles two slots.  No gathered copy of the rows exists for this product: the row's eight byte offsets come from the table
// gsf_stats0_kernel wrote, two 16-byte loads per staged row (looking the documents up here made row() too large to inline into the
// GEMM's chunk set-up, and the row descriptors went to scratch).
struct AGroupLN {
  const float* x;          // [n_docs][F]
  const float* gb;         // the flat parameter vector (gamma at g_off, beta at b_off), gb_floats long
  int64_t n_docs, gb_floats;
  const float* mean;       // [R]
  const float* rstd;       // [R]
  const uint32_t* slots;   // [R][GSF_MAX_GROUP]: the byte offset of slot j's feature row, ULTR_OOB for a PAD and for j >= m
  int64_t R, g_off, b_off;
  int K, F;                // K = m F
  struct Row { u32x4 lo, hi; float mean, rstd; bool in; };
  struct Cols { float4 g, b; };
  __device__ __forceinline__ Row row(int64_t r, int64_t rend) const {
    Row c;
    c.in = r < rend;
    const int64_t rr = c.in ? r : 0;
    const u32x4 oob = {ULTR_OOB, ULTR_OOB, ULTR_OOB, ULTR_OOB};
    const u32x4* sl = reinterpret_cast<const u32x4*>(slots + rr * GSF_MAX_GROUP);
    const u32x4 lo = sl[0], hi = sl[1];
    c.lo = c.in ? lo : oob;
    c.hi = c.in ? hi : oob;
    c.mean = c.in ? mean[rr] : 0.f;
    c.rstd = c.in ? rstd[rr] : 0.f;
    return c;
  }
  __device__ __forceinline__ float4 raw(const Row& c, int k) const {
    const int slot = k / F;
    unsigned o = c.lo.x;
    o = slot == 1 ? c.lo.y : o; o = slot == 2 ? c.lo.z : o; o = slot == 3 ? c.lo.w : o; o = slot == 4 ? c.hi.x : o;
    o = slot == 5 ? c.hi.y : o; o = slot == 6 ? c.hi.z : o; o = slot == 7 ? c.hi.w : o;
    return buf_ld4(make_src(x, n_docs * F), (o != ULTR_OOB && k < K) ? o + (unsigned)(k - slot * F) * 4u : ULTR_OOB);
  }
  __device__ __forceinline__ Cols cols(int k) const {
    Cols o;
    const Src g = make_src(gb, gb_floats);
    o.g = buf_ld4(g, k < K ? (unsigned)((g_off + k) * 4) : ULTR_OOB);
    o.b = buf_ld4(g, k < K ? (unsigned)((b_off + k) * 4) : ULTR_OOB);
    return o;
  }
  // rows past R and columns past K come out as exact zeros (they meet finite B values): gamma = beta = 0 past K, rstd = 0 and beta
  // masked past R
  __device__ __forceinline__ float4 finish(const Row& c, const Cols& o, int, float4 v) const {
    const float mk = c.in ? 1.f : 0.f;
    return make_float4((v.x - c.mean) * c.rstd * o.g.x + mk * o.b.x, (v.y - c.mean) * c.rstd * o.g.y + mk * o.b.y,
                       (v.z - c.mean) * c.rstd * o.g.z + mk * o.b.z, (v.w - c.mean) * c.rstd * o.g.w + mk * o.b.w);
  }
};

unsigned rows4(int64_t T) { return (unsigned)((T + 3) / 4); }

int size_query(const ultr_gsf_desc* c, int64_t B, int64_t L, int64_t T, bool train, GsfPlan& p) {
  const int rc = gsf_check_desc(c);
  if (rc != 0) return rc;
  if (B <= 0 || L <= 0 || T <= 0) return ULTR_E_BADARG;
  gsf_make_plan(c, B, L, T, train, p);
  return 0;
}

}  // namespace

extern "C" {

int64_t ultr_gsf_param_count(const ultr_gsf_desc* c) {
  if (!gsf_is_model(c)) return 0;
  GsfPlan p;
  gsf_param_layout(c, p);
  return p.P;
}

int ultr_gsf_param_offsets(const ultr_gsf_desc* c, int64_t* offsets) {
  if (!gsf_is_model(c) || offsets == nullptr) return ULTR_E_BADARG;
  GsfPlan p;
  gsf_param_layout(c, p);
  for (int j = 0; j < p.nl; ++j) {
    offsets[4 * j + 0] = p.off_g[j];
    offsets[4 * j + 1] = p.off_b[j];
    offsets[4 * j + 2] = p.off_w[j];
    offsets[4 * j + 3] = p.off_c[j];
  }
  return 0;
}

int64_t ultr_gsf_saved_bytes(const ultr_gsf_desc* c, int64_t n_rows) {
  GsfPlan p;
  const int rc = size_query(c, n_rows, n_rows, n_rows, true, p);
  return rc != 0 ? rc : p.saved_floats * 4;
}

int64_t ultr_gsf_score_bytes(const ultr_gsf_desc* c, int64_t n_rows) {
  GsfPlan p;
  const int rc = size_query(c, n_rows, n_rows, n_rows, false, p);
  return rc != 0 ? rc : p.score_floats * 4;
}

int64_t ultr_gsf_workspace_bytes(const ultr_gsf_desc* c, int32_t batch, int32_t list_size) {
  GsfPlan p;
  const int rc = size_query(c, batch, list_size, (int64_t)batch * list_size, true, p);
  return rc != 0 ? rc : p.ws_floats * 4;
}

int ultr_gsf_shuffle(uint64_t seed, uint64_t step, int32_t batch, int32_t list_size, int32_t* perm, void* stream) {
  if (perm == nullptr || batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  hipLaunchKernelGGL(gsf_shuffle_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, seed, step, (int)batch,
                     (int)list_size, perm);
  return (int)hipGetLastError();
}

int ultr_gsf_forward(const ultr_gsf_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                     const int32_t* perm, int32_t batch, int32_t list_size, float* scores, void* saved, void* work, void* stream) {
  const int rc = gsf_check_desc(c);
  if (rc == ULTR_E_BADARG) return rc;
  if (!params || !docids || !scores || (!saved && !work) || batch <= 0 || list_size <= 0 || n_docs < 0 || (n_docs > 0 && !features))
    return ULTR_E_BADARG;
  if (rc != 0) return rc;
  const bool train = saved != nullptr;
  GsfPlan p;
  gsf_make_plan(c, batch, list_size, (int64_t)batch * list_size, train, p);
  if (!gsf_sizes_fit(p, n_docs)) return ULTR_E_UNSUPPORTED;
  float* sv = (float*)(train ? saved : work);
  if (!ultr_aligned16(params) || !ultr_aligned16(sv) || !ultr_aligned16(features)) return ULTR_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int B = p.B, L = p.L, top = p.nl - 1;
  const int64_t T = p.T;
  uint32_t* slots = (uint32_t*)(sv + p.s_slots);
  hipError_t err;

  hipLaunchKernelGGL(gsf_stats0_kernel, dim3(rows4(T)), dim3(256), 0, st, features, docids, perm, n_docs, B, L, T, p.F, p.m, slots,
                     sv + p.s_mean[0], sv + p.s_rstd[0], train ? sv + p.s_xhat : nullptr);
  AGroupLN a0;
  a0.x = features; a0.gb = params; a0.n_docs = n_docs; a0.gb_floats = p.P; a0.mean = sv + p.s_mean[0]; a0.rstd = sv + p.s_rstd[0];
  a0.slots = slots; a0.R = T; a0.g_off = p.off_g[0]; a0.b_off = p.off_b[0]; a0.K = p.K[0]; a0.F = p.F;
  const ugemm::Dims d0{T, p.M[0], p.K[0], p.K[0]};
  if (top == 0) {  // no hidden layer: the one Linear is the head, m columns of the gathering product
    const ugemm::EBiasAct e{sv + p.s_o, params + p.off_c[0], p.m, -1};
    if ((err = ugemm::run<true>(d0, a0, params + p.off_w[0], e, st)) != hipSuccess) return (int)err;
  } else {
    const ugemm::EBiasAct e{sv + p.s_a[0], params + p.off_c[0], p.M[0], p.act};
    if ((err = ugemm::run<true>(d0, a0, params + p.off_w[0], e, st)) != hipSuccess) return (int)err;
    for (int j = 1; j < top; ++j) {
      hipLaunchKernelGGL(gsf_rowstats_kernel, dim3(rows4(T)), dim3(256), 0, st, sv + p.s_a[j - 1], T, p.K[j], sv + p.s_mean[j],
                         sv + p.s_rstd[j]);
      ugemm::ALayerNorm a;
      a.x = sv + p.s_a[j - 1]; a.gb = params; a.x_rows = T; a.gb_floats = p.P; a.mean = sv + p.s_mean[j]; a.rstd = sv + p.s_rstd[j];
      a.ids = nullptr; a.R = T; a.n_docs = 0; a.g_off = p.off_g[j]; a.b_off = p.off_b[j]; a.K = p.K[j]; a.B = B; a.L = L;
      const ugemm::Dims d{T, p.M[j], p.K[j], p.K[j]};
      const ugemm::EBiasAct e2{sv + p.s_a[j], params + p.off_c[j], p.M[j], p.act};
      if ((err = ugemm::run<true>(d, a, params + p.off_w[j], e2, st)) != hipSuccess) return (int)err;
    }
    hipLaunchKernelGGL(gsf_head_fwd_kernel, dim3(rows4(T)), dim3(256), 0, st, sv + p.s_a[top - 1], T, p.K[top], p.m, params + p.off_g[top],
                       params + p.off_b[top], params + p.off_w[top], params + p.off_c[top], sv + p.s_mean[top], sv + p.s_rstd[top],
                       sv + p.s_o);
  }
  hipLaunchKernelGGL(gsf_fold_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, sv + p.s_o, perm, L, T, p.m, scores);
  return (int)hipGetLastError();
}

int ultr_gsf_backward(const ultr_gsf_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                      const int32_t* perm, int32_t batch, int32_t list_size, const void* saved, const float* dscores, const void* loss_ws,
                      int32_t n_loss_parts, void* workspace, float* grads, void* stream) {
  (void)features; (void)docids;  // (the normalised rows the backward reads were kept by the forward)
  const int rc = gsf_check_desc(c);
  if (rc == ULTR_E_BADARG) return rc;
  if (!params || !saved || !dscores || !workspace || !grads || batch <= 0 || list_size <= 0 || n_docs < 0 || n_loss_parts < 0)
    return ULTR_E_BADARG;
  if (rc != 0) return rc;
  GsfPlan p;
  gsf_make_plan(c, batch, list_size, (int64_t)batch * list_size, true, p);
  if (!gsf_sizes_fit(p, n_docs)) return ULTR_E_UNSUPPORTED;
  if (!ultr_aligned16(params) || !ultr_aligned16(saved) || !ultr_aligned16(workspace) || !ultr_aligned16(grads)) return ULTR_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const float* sv = (const float*)saved;
  float* ws = (float*)workspace;
  const int L = p.L, top = p.nl - 1;
  const int64_t T = p.T;
  hipError_t err;

  float* du = ws + p.w_du;
  hipLaunchKernelGGL(gsf_head_bwd_kernel, dim3(rows4(T)), dim3(256), 0, st, dscores, perm, L, T, p.m, p.K[top], params + p.off_w[top],
                     ws + p.w_do, du);
  SrFoldQueue folds(nullptr, 0);  // every partial sum of this backward is folded by ONE launch at its end (fixed order)
  for (int j = top; j >= 0; --j) {
    const float* dz = j == top ? ws + p.w_do : ws + p.w_dz[j];
    // the layer's input before LayerNorm: the activations below it with their statistics; layer 0: the normalised gathered rows
    const float* X = j == 0 ? sv + p.s_xhat : sv + p.s_a[j - 1];
    const float* mean = j == 0 ? nullptr : sv + p.s_mean[j];
    const float* rstd = j == 0 ? nullptr : sv + p.s_rstd[j];
    {
      RgCsTable tb;  // the three column sums of the layer in one launch
      float* part = ws + p.w_cs[j];
      part += tb.add(folds, dz, nullptr, nullptr, nullptr, T, p.M[j], part, grads + p.off_c[j], st);
      part += tb.add(folds, du, nullptr, nullptr, nullptr, T, p.K[j], part, grads + p.off_b[j], st);
      part += tb.add(folds, du, X, mean, rstd, T, p.K[j], part, grads + p.off_g[j], st);
      tb.launch(st);
    }
    rg_wgrad(folds, dz, p.M[j], X, p.K[j], T, 0, mean, rstd, params + p.off_g[j], params + p.off_b[j], ws + p.w_wp[j], grads + p.off_w[j], st);
    if (j > 0) {  // through LayerNorm_j and the activation below it, then the data gradient of Linear_{j-1} (layer 0: for gamma / beta only)
      float* dzb = ws + p.w_dz[j - 1];
      hipLaunchKernelGGL(gsf_ln_bwd_kernel, dim3(rows4(T)), dim3(256), 0, st, du, X, mean, rstd, params + p.off_g[j], T, p.K[j], p.act, dzb);
      const ugemm::APlain a{dzb, T, p.M[j - 1], p.M[j - 1]};
      const ugemm::Dims d{T, p.K[j - 1], p.M[j - 1], p.K[j - 1]};
      const ugemm::EStore e{du, nullptr, p.K[j - 1], 0};
      if ((err = ugemm::run<false>(d, a, params + p.off_w[j - 1], e, st)) != hipSuccess) return (int)err;
    }
  }
  rg_fold_all(folds, loss_ws, n_loss_parts, list_size, grads + p.P, st);
  return (int)hipGetLastError();
}

}  // extern "C"
