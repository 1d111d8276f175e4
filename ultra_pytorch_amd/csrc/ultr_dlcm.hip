// ultr_dlcm.hip - the DLCM ranking model (include/ultr_hip.h: ultr_dlcm_*): LayerNorm -> a one-layer GRU read from the last position to
// the first -> the local ranking function of the paper's eq. 6.  Geometry and buffer layouts: ultr_dlcm_plan.h; DESIGN.md section 3d.
//
//   forward   row statistics -> gi = LN(x) . W_ih^T + b_ih (ONE ugemm::run over all B L tokens, the gathering LayerNorm producer) ->
//             dl_gru_fwd_kernel (ONE launch walks the positions) -> W_phi s + b_phi (ugemm) -> dl_head_fwd_kernel (tanh, m, scores)
//   backward  dl_head_bwd_kernel (dm, dM, dv partials) -> ds = dM . W_phi (ugemm) -> dl_gru_bwd_kernel (ONE launch, the other way,
//             carrying dh; writes the gate gradients) -> d xh = dGi . W_ih (ugemm) -> column sums per row chunk (biases, gamma / beta) ->
//             dW_phi (ugemm, a transposing A producer) -> dW_ih, dW_hh (rg_wgrad: the tokens split over the grid) -> ONE fold
//             launch (the splits and chunks, dv, the loss partials of the step tail)
//
// The recurrent kernels: lists are independent, so a workgroup owns 16 lists (the rows of a v_mfma_f32_16x16x4_f32 tile), keeps their
// state in LDS and needs no grid barrier.  A wave owns column tiles of 16 hidden units and computes the r, z and n products of a tile
// into three accumulators, so the gate arithmetic runs on the lane that holds the products.  W_hh is streamed from L2 at every position
// (3 H H floats: 222 KB at H = 136, more than the LDS holds next to the state).  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/ultr_hip.h"
#include "ultr_device.h"
#include "ultr_dlcm_plan.h"
#include "ultr_gemm.h"
#include "ultr_plan.h"
#include "ultr_rowgrad.h"

namespace {

__device__ __forceinline__ float dl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- row statistics of the gathered feature rows (one wave per token; PAD = the zero row: mean 0, rstd 1 / sqrt(eps)) -------------------
__global__ __launch_bounds__(256) void dl_rowstats_kernel(const float* __restrict__ feats, const int32_t* __restrict__ docids, int64_t n_docs,
                                                          int B, int L, int64_t T, int F, float* __restrict__ mean_out,
                                                          float* __restrict__ rstd_out, float* __restrict__ xhat /* NULL: scoring */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  if (n >= T) return;
  const int bb = (int)(n / L), ll = (int)(n % L);
  const int id = docids[(int64_t)ll * B + bb];
  const float* ra = (id >= 0 && id < n_docs) ? feats + (int64_t)id * F : nullptr;
  float s = 0.f;
  for (int c = lane; c < F; c += 64) s += ra ? ra[c] : 0.f;
  const float mean = wave_sum(s) / (float)F;
  float q = 0.f;
  for (int c = lane; c < F; c += 64) {
    const float d = (ra ? ra[c] : 0.f) - mean;
    q += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)F + ULTR_LN_EPS);
  if (xhat != nullptr)
    for (int c = lane; c < F; c += 64) xhat[n * F + c] = ((ra ? ra[c] : 0.f) - mean) * rstd;
  if (lane == 0) {
    mean_out[n] = mean;
    rstd_out[n] = rstd;
  }
}

// ---- the recurrence, forward: positions L-1 .. 0 -----------------------------------------------------------------------------------------
// LDS: h [2][16][Hp + 8] (the state read by this position and the one it writes; columns H .. Hp and the rows of missing lists stay zero).
// Matrix-core operands: lane (i, q) supplies A = h[list i][k0 + 4 q + s] and B = W_hh[gate row of column i][k0 + 4 q + s] for the four
// steps s of a block of 16 contraction indices (both read as one 16-byte piece), and receives D[list 4 q + r][column i].
__global__ __launch_bounds__(DL_WAVES * 64) void dl_gru_fwd_kernel(const float* __restrict__ params, int64_t off_whh, int64_t off_bhh,
                                                                   const float* __restrict__ gi, float* __restrict__ o,
                                                                   float* __restrict__ gates /* NULL: scoring */, int B, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Hp = (H + 15) / 16 * 16, LDH = Hp + 8, nct = Hp / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  for (int e = tid; e < 2 * DL_LISTS * LDH; e += DL_WAVES * 64) smem[e] = 0.f;
  lds_barrier();
  const int b0 = blockIdx.x * DL_LISTS;
  const Src wsrc = make_src(params + off_whh, (int64_t)3 * H * H);
  const float* bhh = params + off_bhh;
  int cur = 0;
  for (int l = L - 1; l >= 0; --l) {
    const float* hc = smem + cur * DL_LISTS * LDH;
    float* hn = smem + (cur ^ 1) * DL_LISTS * LDH;
    for (int ct = wave; ct < nct; ct += DL_WAVES) {
      const int col = ct * 16 + i;
      const bool colok = col < H;
      // the input projections of this lane's four lists: requested in front of the products
      float gir[4], giz[4], gin[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + 4 * q + r;
        const bool ok = colok && b < B;
        const int64_t t = (int64_t)b * L + l;
        gir[r] = ok ? gi[t * 3 * H + col] : 0.f;
        giz[r] = ok ? gi[t * 3 * H + H + col] : 0.f;
        gin[r] = ok ? gi[t * 3 * H + 2 * H + col] : 0.f;
      }
      f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
      for (int k0 = 0; k0 < Hp; k0 += 16) {
        const int kk = k0 + 4 * q;
        const float4 a = ld4(hc + i * LDH + kk);
        const bool ok = colok && kk < H;  // (H is a multiple of 4: the piece is inside the row or past it)
        const float4 wr = buf_ld4(wsrc, ok ? (unsigned)(((int64_t)col * H + kk) * 4) : ULTR_OOB);
        const float4 wz = buf_ld4(wsrc, ok ? (unsigned)(((int64_t)(H + col) * H + kk) * 4) : ULTR_OOB);
        const float4 wn = buf_ld4(wsrc, ok ? (unsigned)(((int64_t)(2 * H + col) * H + kk) * 4) : ULTR_OOB);
        ar = mfma16(a.x, wr.x, ar); ar = mfma16(a.y, wr.y, ar); ar = mfma16(a.z, wr.z, ar); ar = mfma16(a.w, wr.w, ar);
        az = mfma16(a.x, wz.x, az); az = mfma16(a.y, wz.y, az); az = mfma16(a.z, wz.z, az); az = mfma16(a.w, wz.w, az);
        an = mfma16(a.x, wn.x, an); an = mfma16(a.y, wn.y, an); an = mfma16(a.z, wn.z, an); an = mfma16(a.w, wn.w, an);
      }
      if (colok) {
        const float br = bhh[col], bz = bhh[H + col], bn = bhh[2 * H + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int list = 4 * q + r, b = b0 + list;
          if (b < B) {
            const int64_t t = (int64_t)b * L + l;
            const float rr = dl_sigmoid(gir[r] + (ar[r] + br));
            const float zz = dl_sigmoid(giz[r] + (az[r] + bz));
            const float hh = an[r] + bn;
            const float nn = tanhf(gin[r] + rr * hh);
            const float hnew = (1.0f - zz) * nn + zz * hc[list * LDH + col];
            hn[list * LDH + col] = hnew;
            o[t * H + col] = hnew;
            if (gates != nullptr) {
              float* g = gates + t * 4 * H + col;
              g[0] = rr;
              g[H] = zz;
              g[2 * H] = nn;
              g[3 * H] = hh;
            }
          }
        }
      }
    }
    lds_barrier();
    cur ^= 1;
  }
}

// ---- the recurrence, backward: positions 0 .. L-1, carrying dh ---------------------------------------------------------------------------
// LDS: dg [16][3 Hp + 8] (this position's gradients of the three hidden products, the A operand), dh [16][Hp + 8] (the carried state
// gradient; between the two phases of a position it holds the part that bypasses the products, dh' z).  The product dg . W_hh contracts over
// W_hh's ROWS: lane (i, q) supplies B = W_hh[gate row k0 + 4 q + s][column i], four 4-byte loads that 16 lanes make contiguous.
// DH_GLOBAL: dh lives in the workspace instead (hidden sizes whose dg and dh do not both fit the LDS).  Every entry of dh is read and
// written by ONE lane throughout, so that copy needs no barrier and no coherence; the launcher zeroes it.
template <bool DH_GLOBAL>
__global__ __launch_bounds__(DL_WAVES * 64) void dl_gru_bwd_kernel(const float* __restrict__ params, int64_t off_whh, const float* __restrict__ o,
                                                                   const float* __restrict__ gates, const float* __restrict__ dscores,
                                                                   const float* __restrict__ m, const float* __restrict__ ds,
                                                                   float* __restrict__ dGi, float* __restrict__ dGh, float* dh_ws, int B, int L,
                                                                   int H) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Hp = (H + 15) / 16 * 16, LDH = Hp + 8, LDG = 3 * Hp + 8, nct = Hp / 16;
  float* dg = smem;
  float* dh;
  if constexpr (DH_GLOBAL) dh = dh_ws + (int64_t)blockIdx.x * DL_LISTS * LDH;
  else dh = smem + DL_LISTS * LDG;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  for (int e = tid; e < DL_LISTS * (LDG + (DH_GLOBAL ? 0 : LDH)); e += DL_WAVES * 64) smem[e] = 0.f;
  lds_barrier();
  const int b0 = blockIdx.x * DL_LISTS;
  const Src wsrc = make_src(params + off_whh, (int64_t)3 * H * H);
  for (int l = 0; l < L; ++l) {
    // phase 1: through the gate arithmetic (a lane owns the same (list, column) entries of dh in both phases)
    for (int ct = wave; ct < nct; ct += DL_WAVES) {
      const int col = ct * 16 + i;
      if (col < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int list = 4 * q + r, b = b0 + list;
          if (b < B) {
            const int64_t t = (int64_t)b * L + l;
            float dout = dscores[t] * m[(int64_t)b * H + col];
            if (l == 0) dout += ds[(int64_t)b * H + col];
            const float dhp = dh[list * LDH + col] + dout;
            const float* g = gates + t * 4 * H + col;
            const float rr = g[0], zz = g[H], nn = g[2 * H], hh = g[3 * H];
            const float hprev = (l + 1 < L) ? o[(t + 1) * H + col] : 0.f;
            const float dn = dhp * (1.0f - zz), dz = dhp * (hprev - nn);
            const float dpn = dn * (1.0f - nn * nn);
            const float dpr = dpn * hh * (rr * (1.0f - rr));
            const float dpz = dz * (zz * (1.0f - zz));
            const float dph = dpn * rr;
            float* gi_ = dGi + t * 3 * H + col;
            gi_[0] = dpr; gi_[H] = dpz; gi_[2 * H] = dpn;
            float* gh_ = dGh + t * 3 * H + col;
            gh_[0] = dpr; gh_[H] = dpz; gh_[2 * H] = dph;
            dg[list * LDG + col] = dpr;
            dg[list * LDG + Hp + col] = dpz;
            dg[list * LDG + 2 * Hp + col] = dph;
            dh[list * LDH + col] = dhp * zz;
          }
        }
      }
    }
    lds_barrier();
    // phase 2: dh = dh' z + dg . W_hh
    for (int ct = wave; ct < nct; ct += DL_WAVES) {
      const int col = ct * 16 + i;
      const bool colok = col < H;
      f32x4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = dh[(4 * q + r) * LDH + col];
      for (int k0 = 0; k0 < 3 * Hp; k0 += 16) {
        const float4 a = ld4(dg + i * LDG + k0 + 4 * q);
        const int g = k0 / Hp, c0 = k0 - g * Hp + 4 * q;
        float w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int kc = c0 + s;
          w[s] = buf_ld1(wsrc, (colok && kc < H) ? (unsigned)((((int64_t)g * H + kc) * H + col) * 4) : ULTR_OOB);
        }
        acc = mfma16(a.x, w[0], acc); acc = mfma16(a.y, w[1], acc); acc = mfma16(a.z, w[2], acc); acc = mfma16(a.w, w[3], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[(4 * q + r) * LDH + col] = acc[r];
    }
    lds_barrier();
  }
}

// ---- the head: one workgroup per list ----------------------------------------------------------------------------------------------------
// M = tanh(pre) in place, m = sum_j v_j M_j, score_l = o_l . m (a wave per position)
__global__ __launch_bounds__(256) void dl_head_fwd_kernel(float* __restrict__ M, const float* __restrict__ v, const float* __restrict__ o,
                                                          float* __restrict__ m_out, float* __restrict__ scores, int L, int H, int heads) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // m [H]
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* Mb = M + (int64_t)b * heads * H;
  for (int c = threadIdx.x; c < H; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < heads; ++j) {
      const float t = tanhf(Mb[(int64_t)j * H + c]);
      Mb[(int64_t)j * H + c] = t;
      acc = fmaf(v[j], t, acc);
    }
    smem[c] = acc;
    m_out[(int64_t)b * H + c] = acc;
  }
  __syncthreads();
  for (int l = wave; l < L; l += 4) {
    const float* ol = o + ((int64_t)b * L + l) * H;
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s = fmaf(ol[c], smem[c], s);
    s = wave_sum(s);
    if (lane == 0) scores[(int64_t)b * L + l] = s;
  }
}
// dm = sum_l dscore_l o_l; d pre = v_j dm (1 - M^2); this list's part of dv_j = dm . M_j   (d o_l = dscore_l m is formed by the recurrence)
__global__ __launch_bounds__(256) void dl_head_bwd_kernel(const float* __restrict__ M, const float* __restrict__ v, const float* __restrict__ o,
                                                          const float* __restrict__ dscores, float* __restrict__ dM, float* __restrict__ dvpart,
                                                          int L, int H, int heads) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // dm [H]
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* Mb = M + (int64_t)b * heads * H;
  for (int c = threadIdx.x; c < H; c += 256) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc = fmaf(dscores[(int64_t)b * L + l], o[((int64_t)b * L + l) * H + c], acc);
    smem[c] = acc;
    for (int j = 0; j < heads; ++j) {
      const float t = Mb[(int64_t)j * H + c];
      dM[((int64_t)b * heads + j) * H + c] = v[j] * acc * (1.0f - t * t);
    }
  }
  __syncthreads();
  for (int j = wave; j < heads; j += 4) {
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s = fmaf(smem[c], Mb[(int64_t)j * H + c], s);
    s = wave_sum(s);
    if (lane == 0) dvpart[(int64_t)b * heads + j] = s;
  }
}

// ---- pieces for ugemm::run ---------------------------------------------------------------------------------------------------------------
// A[r][k] = src[k][r]: the transpose of a row-major [K][ld] matrix (weight gradients: the contraction runs over the tokens).  mask_L != 0:
// source rows k with k % mask_L == mask_L - 1 read as zeros (the last position of every list has no previous state).
struct ATrans {
  const float* a;
  int64_t K;
  int ld, mask_L;
  struct Row { unsigned off; };
  struct Cols {};
  __device__ __forceinline__ Row row(int64_t r, int64_t rend) const { return Row{r < rend ? (unsigned)(r * 4) : ULTR_OOB}; }
  __device__ __forceinline__ float4 raw(const Row& c, int k) const {
    const Src s = make_src(a, K * ld);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t kk = (int64_t)k + j;
      const bool ok = c.off != ULTR_OOB && kk < K && (mask_L == 0 || (int)(kk % mask_L) != mask_L - 1);
      v[j] = buf_ld1(s, ok ? c.off + (unsigned)(kk * ld * 4) : ULTR_OOB);
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
  __device__ __forceinline__ Cols cols(int) const { return Cols{}; }
  __device__ __forceinline__ float4 finish(const Row&, const Cols&, int, float4 v) const { return v; }
};
hipError_t dl_set_lds(const void* kern, std::atomic<int64_t>* set, int64_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ugemm::UGEMM_MAX_DEV) dev = 0;
  if (bytes <= 64 * 1024 || set[dev].load(std::memory_order_acquire) >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) set[dev].store(bytes, std::memory_order_release);
  return e;
}

}  // namespace

extern "C" {

int ultr_dlcm_param_offsets(const ultr_dlcm_desc* c, int64_t* offsets) {
  if (c == nullptr || offsets == nullptr || c->feature_size <= 0 || c->hidden_size <= 0 || c->num_heads <= 0) return ULTR_E_BADARG;
  DlPlan p;
  dl_param_layout(c, p);
  const int64_t o[10] = {p.p_gamma, p.p_beta, p.p_wih, p.p_whh, p.p_bih, p.p_bhh, p.p_wphi, p.p_bphi, p.p_v, p.P};
  for (int k = 0; k < 10; ++k) offsets[k] = o[k];
  return 0;
}

int64_t ultr_dlcm_saved_bytes(const ultr_dlcm_desc* c, int64_t n_rows) {
  const int rc = dl_check_desc(c);
  if (rc != 0) return rc;
  if (n_rows <= 0) return ULTR_E_BADARG;
  DlPlan p;
  dl_make_plan(c, n_rows, n_rows, n_rows, p);
  return p.saved_floats * 4;
}

int64_t ultr_dlcm_score_bytes(const ultr_dlcm_desc* c, int64_t n_rows) {
  const int rc = dl_check_desc(c);
  if (rc != 0) return rc;
  if (n_rows <= 0) return ULTR_E_BADARG;
  DlPlan p;
  dl_make_plan(c, n_rows, n_rows, n_rows, p);
  return p.score_floats * 4;
}

int64_t ultr_dlcm_workspace_bytes(const ultr_dlcm_desc* c, int32_t batch, int32_t list_size) {
  const int rc = dl_check_desc(c);
  if (rc != 0) return rc;
  if (batch <= 0 || list_size <= 0) return ULTR_E_BADARG;
  DlPlan p;
  dl_make_plan(c, batch, list_size, (int64_t)batch * list_size, p);
  return p.ws_floats * 4;
}

int ultr_dlcm_forward(const ultr_dlcm_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                      int32_t batch, int32_t list_size, float* scores, void* saved, void* work, void* stream) {
  int rc = dl_check_desc(c);
  if (rc == ULTR_E_BADARG) return rc;
  if (!params || !docids || !scores || (!saved && !work) || batch <= 0 || list_size <= 0 || n_docs < 0 || (n_docs > 0 && !features))
    return ULTR_E_BADARG;
  if (rc != 0) return rc;
  DlPlan p;
  dl_make_plan(c, batch, list_size, (int64_t)batch * list_size, p);
  if (!dl_sizes_fit(p, n_docs) || p.lds_fwd > DL_LDS_MAX) return ULTR_E_UNSUPPORTED;
  float* sv = (float*)(saved ? saved : work);
  if (!ultr_aligned16(params) || !ultr_aligned16(sv) || !ultr_aligned16(features)) return ULTR_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const bool train = saved != nullptr;
  const int F = p.F, H = p.H, hH = p.heads * p.H, B = p.B, L = p.L;
  const int64_t T = p.T;

  hipLaunchKernelGGL(dl_rowstats_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, features, docids, n_docs, B, L, T, F, sv + p.s_mean,
                     sv + p.s_rstd, train ? sv + p.s_xhat : nullptr);
  {  // gi = LN(x) . W_ih^T + b_ih
    ugemm::ALayerNorm a;
    a.x = features; a.gb = params; a.x_rows = n_docs; a.gb_floats = p.P; a.mean = sv + p.s_mean; a.rstd = sv + p.s_rstd; a.ids = docids;
    a.R = T; a.n_docs = n_docs; a.g_off = p.p_gamma; a.b_off = p.p_beta; a.K = F; a.B = B; a.L = L;
    const ugemm::Dims d{T, 3 * H, F, F};
    const ugemm::EBiasAct e{sv + p.s_gi, params + p.p_bih, 3 * H, -1};
    const hipError_t err = ugemm::run<true>(d, a, params + p.p_wih, e, st);
    if (err != hipSuccess) return (int)err;
  }
  {
    static std::atomic<int64_t> set[ugemm::UGEMM_MAX_DEV];
    const hipError_t err = dl_set_lds(reinterpret_cast<const void*>(dl_gru_fwd_kernel), set, p.lds_fwd);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(dl_gru_fwd_kernel, dim3((unsigned)((B + DL_LISTS - 1) / DL_LISTS)), dim3(DL_WAVES * 64), (size_t)p.lds_fwd, st, params,
                       p.p_whh, p.p_bhh, sv + p.s_gi, sv + p.s_o, train ? sv + p.s_gates : nullptr, B, L, H);
  }
  {  // W_phi s + b_phi, s = o_0 of every list
    const ugemm::APlain a{sv + p.s_o, (int64_t)B, H, L * H};
    const ugemm::Dims d{(int64_t)B, hH, H, H};
    const ugemm::EBiasAct e{sv + p.s_M, params + p.p_bphi, hH, -1};
    const hipError_t err = ugemm::run<true>(d, a, params + p.p_wphi, e, st);
    if (err != hipSuccess) return (int)err;
  }
  hipLaunchKernelGGL(dl_head_fwd_kernel, dim3((unsigned)B), dim3(256), (size_t)H * 4, st, sv + p.s_M, params + p.p_v, sv + p.s_o, sv + p.s_m,
                     scores, L, H, p.heads);
  return (int)hipGetLastError();
}

int ultr_dlcm_backward(const ultr_dlcm_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                       int32_t batch, int32_t list_size, const void* saved, const float* dscores, const void* loss_ws,
                       int32_t n_loss_parts, void* workspace, float* grads, void* stream) {
  (void)features; (void)docids;  // (the normalised rows the backward reads were kept by the forward)
  int rc = dl_check_desc(c);
  if (rc == ULTR_E_BADARG) return rc;
  if (!params || !saved || !dscores || !workspace || !grads || batch <= 0 || list_size <= 0 || n_docs < 0 || n_loss_parts < 0)
    return ULTR_E_BADARG;
  if (rc != 0) return rc;
  DlPlan p;
  dl_make_plan(c, batch, list_size, (int64_t)batch * list_size, p);
  if (!dl_sizes_fit(p, n_docs) || p.lds_bwd > DL_LDS_MAX) return ULTR_E_UNSUPPORTED;
  if (!ultr_aligned16(params) || !ultr_aligned16(saved) || !ultr_aligned16(workspace) || !ultr_aligned16(grads)) return ULTR_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const float* sv = (const float*)saved;
  float* ws = (float*)workspace;
  const int F = p.F, H = p.H, hH = p.heads * p.H, B = p.B, L = p.L;
  const int64_t T = p.T;
  hipError_t err;

  hipLaunchKernelGGL(dl_head_bwd_kernel, dim3((unsigned)B), dim3(256), (size_t)H * 4, st, sv + p.s_M, params + p.p_v, sv + p.s_o, dscores,
                     ws + p.w_dM, ws + p.w_dv, L, H, p.heads);
  {  // ds = dM . W_phi
    const ugemm::APlain a{ws + p.w_dM, (int64_t)B, hH, hH};
    const ugemm::Dims d{(int64_t)B, H, hH, H};
    const ugemm::EStore e{ws + p.w_ds, nullptr, H, 0};
    if ((err = ugemm::run<false>(d, a, params + p.p_wphi, e, st)) != hipSuccess) return (int)err;
  }
  {
    static std::atomic<int64_t> set[2][ugemm::UGEMM_MAX_DEV];
    const dim3 grid((unsigned)((B + DL_LISTS - 1) / DL_LISTS)), block(DL_WAVES * 64);
    if (p.dh_global) {
      if ((err = dl_set_lds(reinterpret_cast<const void*>(dl_gru_bwd_kernel<true>), set[1], p.lds_bwd)) != hipSuccess) return (int)err;
      if ((err = hipMemsetAsync(ws + p.w_dh, 0, (size_t)p.dh_floats * sizeof(float), st)) != hipSuccess) return (int)err;
      hipLaunchKernelGGL(dl_gru_bwd_kernel<true>, grid, block, (size_t)p.lds_bwd, st, params, p.p_whh, sv + p.s_o, sv + p.s_gates, dscores,
                         sv + p.s_m, ws + p.w_ds, ws + p.w_dgi, ws + p.w_dgh, ws + p.w_dh, B, L, H);
    } else {
      if ((err = dl_set_lds(reinterpret_cast<const void*>(dl_gru_bwd_kernel<false>), set[0], p.lds_bwd)) != hipSuccess) return (int)err;
      hipLaunchKernelGGL(dl_gru_bwd_kernel<false>, grid, block, (size_t)p.lds_bwd, st, params, p.p_whh, sv + p.s_o, sv + p.s_gates, dscores,
                         sv + p.s_m, ws + p.w_ds, ws + p.w_dgi, ws + p.w_dgh, (float*)nullptr, B, L, H);
    }
  }
  {  // d xh = dGi . W_ih
    const ugemm::APlain a{ws + p.w_dgi, T, 3 * H, 3 * H};
    const ugemm::Dims d{T, F, 3 * H, F};
    const ugemm::EStore e{ws + p.w_dxh, nullptr, F, 0};
    if ((err = ugemm::run<false>(d, a, params + p.p_wih, e, st)) != hipSuccess) return (int)err;
  }
  SrFoldQueue folds(nullptr, 0);  // every partial sum of this backward is folded by ONE launch at its end (fixed order)
  {
    RgCsTable tb;  // every column sum of this backward in one launch
    float* part = ws + p.w_cspart;
    part += tb.add(folds, ws + p.w_dgi, nullptr, nullptr, nullptr, T, 3 * H, part, grads + p.p_bih, st);
    part += tb.add(folds, ws + p.w_dgh, nullptr, nullptr, nullptr, T, 3 * H, part, grads + p.p_bhh, st);
    part += tb.add(folds, ws + p.w_dM, nullptr, nullptr, nullptr, B, hH, part, grads + p.p_bphi, st);
    part += tb.add(folds, ws + p.w_dxh, nullptr, nullptr, nullptr, T, F, part, grads + p.p_beta, st);
    part += tb.add(folds, ws + p.w_dxh, sv + p.s_xhat, nullptr, nullptr, T, F, part, grads + p.p_gamma, st);
    tb.launch(st);
  }
  {  // dW_phi = dM^T . s (the contraction is the batch: short)
    const ATrans a{ws + p.w_dM, (int64_t)B, hH, 0};
    const ugemm::Dims d{(int64_t)hH, H, B, L * H};
    const ugemm::EStore e{grads + p.p_wphi, nullptr, H, 0};
    if ((err = ugemm::run<false>(d, a, sv + p.s_o, e, st)) != hipSuccess) return (int)err;
  }
  // dW_ih = dGi^T . xh, xh = xhat gamma + beta formed as the operand is read
  rg_wgrad(folds, ws + p.w_dgi, 3 * H, sv + p.s_xhat, F, T, 0, nullptr, nullptr, params + p.p_gamma, params + p.p_beta, ws + p.w_wpart_ih,
           grads + p.p_wih, st);
  // dW_hh = dGh^T . h_prev: token t's previous state is o[t + 1], none at a list's last position (the very last token among them)
  rg_wgrad(folds, ws + p.w_dgh, 3 * H, sv + p.s_o + H, H, T - 1, L, nullptr, nullptr, nullptr, nullptr, ws + p.w_wpart_hh, grads + p.p_whh,
           st);
  folds.add(ws + p.w_dv, (int64_t)p.heads, B, p.heads, grads + p.p_v, st, /*own_buffer=*/true);
  rg_fold_all(folds, loss_ws, n_loss_parts, list_size, grads + p.P, st);
  return (int)hipGetLastError();
}

}  // extern "C"
