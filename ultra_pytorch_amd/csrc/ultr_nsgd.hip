// ultr_nsgd.hip - NSGD's noise and its memory of losing directions (reference nsgd.py; Wang et al., SIGIR 2018).  The rest of an NSGD
// step is MGD's (ultr_dbgd.hip): R + 1 forwards, the multileave or the per-ranker NDCGs, dbgd_grad_kernel and the shared update.
//
// The noise of ranker r on Linear tensor t (a weight [out, in] or a bias [out] of the flat DNN vector), u = normalize(P_t z): z are
// Philox normals over the whole tensor, P_t the orthogonal projection onto the complement of the memory rows restricted to t, and
// normalize the reference's whole-tensor x / sqrt(max(sum x^2, 1e-12)).  With m_i the memory rows and G their Gram matrix,
// P_t z = z - sum_i alpha_i m_i with G alpha = (<z, m_i>)_i solved over the rows a pivoted Cholesky of G keeps.  Four launches:
//   nsgd_dot_kernel      per chunk of 256 elements of one tensor: z (written to noise), the partial Gram matrix and <z_r, m_i> in fp64
//   nsgd_solve_kernel    per tensor: the fixed-order sum of the partials, the pivoted Cholesky and every ranker's alpha in fp64
//   nsgd_project_kernel  per chunk: v = z - sum_i alpha_i m_i (written to noise) and each ranker's partial sum of squares
//   nsgd_finish_kernel   per chunk (and per layer for the LayerNorm entries): u = v / sqrt(max(sum v^2, 1e-12)), the candidates
// and after the winners nsgd_memory_kernel: memory row r = noise_r if ranker r + 1 lost, else 0.
// Every reduction has a fixed order over a fixed chunking: a step is a pure function of (seed, step, params, memory).  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ultr_hip.h"
#include "ultr_dbgd.h"
#include "ultr_device.h"
#include "ultr_plan.h"

#define NSGD_NOISE_TAG 0x0E56D001u
#define NSGD_CHUNK 256                             // elements per workgroup of the dot, project, finish and memory kernels
#define NSGD_MAX_R (ULTR_DBGD_MAX_RANKERS - 1)    // memory rows = candidate rankers
#define NSGD_MAX_T (2 * ULTR_MAXL)                 // Linear tensors: a weight and a bias per layer
#define NSGD_PIVOT_TOL 1e-12                       // a pivot below this fraction of the largest memory row's squared norm is dropped

struct NsgdLayout {
  int nl, nt, R, np, nchunks;  // np: partials per chunk, R (R + 1) / 2 Gram entries then R x R <z_r, m_i>
  int64_t P;
  int64_t off[NSGD_MAX_T], len[NSGD_MAX_T];
  int c0[NSGD_MAX_T + 1];  // first chunk of tensor t; c0[nt] = nchunks
  int K[ULTR_MAXL];
  int64_t off_ln[ULTR_MAXL];
  // offsets in doubles into ws: the partials [nchunks, np] at 0, alpha [nt, R, R], zero flags [nt], sums of squares [nchunks, R]
  int64_t ws_coef, ws_flag, ws_ss;
};

__device__ __forceinline__ double wave_sum_f64(double v) {  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int nsgd_tensor(const NsgdLayout& ly, int c) {
  int t = 0;
  while (t < ly.nt - 1 && c >= ly.c0[t + 1]) ++t;
  return t;
}

__device__ __forceinline__ int nsgd_chunk_len(const NsgdLayout& ly, int t, int64_t base) {
  const int64_t rest = ly.off[t] + ly.len[t] - base;
  return rest < NSGD_CHUNK ? (int)rest : NSGD_CHUNK;
}

// the bias of one entry: the reference skips the null space for a tensor with sum(shape) <= 1
__device__ __forceinline__ bool nsgd_scalar(const NsgdLayout& ly, int t) { return (t & 1) && ly.len[t] == 1; }

// grid nchunks, 256 threads (one element each)
__global__ __launch_bounds__(256) void nsgd_dot_kernel(ultr_dbgd_args a, ultr_nsgd_args n, NsgdLayout ly) {
  __shared__ float zs[NSGD_MAX_R][NSGD_CHUNK + 1];  // (+1: the rows of one column fall in different banks)
  __shared__ float ms[NSGD_MAX_R][NSGD_CHUNK + 1];
  __shared__ double red[256];
  const int c = blockIdx.x, tid = threadIdx.x, R = ly.R;
  const int t = nsgd_tensor(ly, c);
  const int64_t base = ly.off[t] + (int64_t)(c - ly.c0[t]) * NSGD_CHUNK, P = ly.P;
  const int len = nsgd_chunk_len(ly, t, base);
  const Philox rng = philox_step_key(a.seed, a.step);
  for (int r = 0; r < R; ++r) {
    float z = 0.f, m = 0.f;
    if (tid < len) {
      const int64_t e = (int64_t)r * P + base + tid;
      z = n.normals_in != nullptr ? n.normals_in[e] : philox_normal(rng, r, base + tid, NSGD_NOISE_TAG);
      m = n.memory[e];
      a.noise[e] = z;
    }
    zs[r][tid] = z;
    ms[r][tid] = m;
  }
  __syncthreads();
  double* part = static_cast<double*>(n.ws) + (int64_t)c * ly.np;
  const int ng = R * (R + 1) / 2;
  // S = 256 / np threads per product (a function of R alone), each over the elements s, s + S, ...; their sums added in order s
  const int S = ly.np < 256 ? 256 / ly.np : 1;
  for (int q = tid; q < ly.np * S; q += 256) {
    const int p = q / S, s0 = q - p * S;
    const float *x, *y;
    if (p < ng) {  // Gram entry (i, k), i <= k, row-major over the upper triangle
      int i = 0, q = p;
      while (q >= R - i) q -= R - i++;
      x = ms[i];
      y = ms[i + q];
    } else {
      const int q = p - ng;
      x = zs[q / R];
      y = ms[q % R];
    }
    double s = 0.0;
    for (int l = s0; l < len; l += S) s += (double)x[l] * (double)y[l];
    if (S == 1)
      part[p] = s;
    else
      red[q] = s;
  }
  if (S > 1) {
    __syncthreads();
    if (tid < ly.np) {
      double s = 0.0;
      for (int k = 0; k < S; ++k) s += red[tid * S + k];
      part[tid] = s;
    }
  }
}

// grid nt, 1024 threads.  The partials of tensor t in a fixed order (lane-strided over its chunks, then the wave's butterfly), the
// pivoted Cholesky of G (one lane: R <= 15), then alpha_r = G^-1 <z_r, m> over the kept rows (lane r).
__global__ __launch_bounds__(1024) void nsgd_solve_kernel(ultr_nsgd_args n, NsgdLayout ly) {
  __shared__ double g[NSGD_MAX_R][NSGD_MAX_R];   // the Gram matrix, then the Schur complement
  __shared__ double d[NSGD_MAX_R][NSGD_MAX_R];   // d[r][i] = <z_r, m_i>
  __shared__ double lc[NSGD_MAX_R][NSGD_MAX_R];  // lc[s][i]: column s of the pivoted factor at row i
  __shared__ double xs[NSGD_MAX_R][NSGD_MAX_R];  // lane r's solve
  __shared__ int piv[NSGD_MAX_R];
  __shared__ int rank_s;
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, R = ly.R;
  const int ng = R * (R + 1) / 2;
  const double* part = static_cast<const double*>(n.ws);
  for (int p = w; p < ly.np; p += 16) {
    double s = 0.0;
    for (int c = ly.c0[t] + lane; c < ly.c0[t + 1]; c += 64) s += part[(int64_t)c * ly.np + p];
    s = wave_sum_f64(s);
    if (lane == 0) {
      if (p < ng) {
        int i = 0, q = p;
        while (q >= R - i) q -= R - i++;
        g[i][i + q] = s;
        g[i + q][i] = s;
      } else {
        d[(p - ng) / R][(p - ng) % R] = s;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    if (!nsgd_scalar(ly, t)) {
      double dmax = 0.0;
      for (int i = 0; i < R; ++i) dmax = fmax(dmax, g[i][i]);
      const double tol = dmax * NSGD_PIVOT_TOL;
      unsigned used = 0u;
      for (; k < R; ++k) {
        int q = -1;
        double best = tol;
        for (int i = 0; i < R; ++i)
          if (!((used >> i) & 1u) && g[i][i] > best) {
            best = g[i][i];
            q = i;
          }
        if (q < 0) break;
        used |= 1u << q;
        piv[k] = q;
        const double l = sqrt(g[q][q]);
        for (int i = 0; i < R; ++i) lc[k][i] = ((used >> i) & 1u) ? 0.0 : g[i][q] / l;
        lc[k][q] = l;
        for (int i = 0; i < R; ++i)
          for (int j = 0; j < R; ++j)
            if (!((used >> i) & 1u) && !((used >> j) & 1u)) g[i][j] -= lc[k][i] * lc[k][j];
      }
    }
    rank_s = k;
    static_cast<double*>(n.ws)[ly.ws_flag + t] = k >= ly.len[t] ? 1.0 : 0.0;  // the kept rows span the tensor: u = 0
  }
  __syncthreads();
  if (tid < R) {
    const int r = tid, k = rank_s;
    double* x = xs[r];
    for (int s = 0; s < k; ++s) {  // L y = d_piv
      double v = d[r][piv[s]];
      for (int b = 0; b < s; ++b) v -= lc[b][piv[s]] * x[b];
      x[s] = v / lc[s][piv[s]];
    }
    for (int s = k - 1; s >= 0; --s) {  // L^T alpha = y
      double v = x[s];
      for (int b = s + 1; b < k; ++b) v -= lc[s][piv[b]] * x[b];
      x[s] = v / lc[s][piv[s]];
    }
    double* coef = static_cast<double*>(n.ws) + ly.ws_coef + ((int64_t)t * R + r) * R;
    for (int i = 0; i < R; ++i) coef[i] = 0.0;
    for (int s = 0; s < k; ++s) coef[piv[s]] = x[s];
  }
}

// grid nchunks, 256 threads (one element each, every ranker)
__global__ __launch_bounds__(256) void nsgd_project_kernel(ultr_dbgd_args a, ultr_nsgd_args n, NsgdLayout ly) {
  __shared__ double cf[NSGD_MAX_R][NSGD_MAX_R];
  __shared__ double red[NSGD_MAX_R][4];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, R = ly.R;
  const int t = nsgd_tensor(ly, c);
  const int64_t base = ly.off[t] + (int64_t)(c - ly.c0[t]) * NSGD_CHUNK, P = ly.P;
  const int len = nsgd_chunk_len(ly, t, base);
  double* ws = static_cast<double*>(n.ws);
  if (tid < R * R) cf[tid / R][tid % R] = ws[ly.ws_coef + (int64_t)t * R * R + tid];
  const bool zero = ws[ly.ws_flag + t] != 0.0;
  __syncthreads();
  const bool live = tid < len;
  float m[NSGD_MAX_R];
#pragma unroll
  for (int i = 0; i < NSGD_MAX_R; ++i) m[i] = (live && i < R) ? n.memory[(int64_t)i * P + base + tid] : 0.f;
  for (int r = 0; r < R; ++r) {
    double ss = 0.0;
    if (live) {
      const int64_t e = (int64_t)r * P + base + tid;
      double v = (double)a.noise[e];
#pragma unroll
      for (int i = 0; i < NSGD_MAX_R; ++i)
        if (i < R) v -= cf[r][i] * (double)m[i];
      const float vf = zero ? 0.f : (float)v;
      a.noise[e] = vf;
      ss = (double)vf * (double)vf;
    }
    ss = wave_sum_f64(ss);
    if (lane == 0) red[r][w] = ss;
  }
  __syncthreads();
  if (tid < R) ws[ly.ws_ss + (int64_t)c * R + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// grid (nchunks + nl, R), 256 threads.  Chunk workgroups: the tensor's sum of squares (fixed order), u and the candidate entries;
// the last nl workgroups: the LayerNorm entries of layer j (no noise).
__global__ __launch_bounds__(256) void nsgd_finish_kernel(ultr_dbgd_args a, ultr_nsgd_args n, NsgdLayout ly) {
  __shared__ float den_s;
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, R = ly.R;
  const int64_t P = ly.P;
  float* __restrict__ u = a.noise + (int64_t)r * P;
  float* __restrict__ th = a.cand_params + (int64_t)r * (a.cand_stride > 0 ? a.cand_stride : P);
  const float rate = a.noise_rate;
  if (c >= ly.nchunks) {
    const int j = c - ly.nchunks;
    for (int k = tid; k < 2 * ly.K[j]; k += 256) {
      const int64_t e = ly.off_ln[j] + k;
      u[e] = 0.f;
      th[e] = a.params[e];
    }
    return;
  }
  const int t = nsgd_tensor(ly, c);
  const int64_t base = ly.off[t] + (int64_t)(c - ly.c0[t]) * NSGD_CHUNK;
  const int len = nsgd_chunk_len(ly, t, base);
  if (n.unit_noise_in != nullptr) {
    if (tid < len) {
      const int64_t e = base + tid;
      const float v = n.unit_noise_in[(int64_t)r * P + e];
      u[e] = v;
      th[e] = a.params[e] + rate * v;
    }
    return;
  }
  const double* ws = static_cast<const double*>(n.ws);
  if (tid < 64) {
    double s = 0.0;
    for (int cc = ly.c0[t] + tid; cc < ly.c0[t + 1]; cc += 64) s += ws[ly.ws_ss + (int64_t)cc * R + r];
    s = wave_sum_f64(s);
    if (tid == 0) den_s = (float)sqrt(fmax(s, 1e-12));
  }
  __syncthreads();
  if (tid < len) {
    const int64_t e = base + tid;
    const float v = u[e] / den_s;  // (0 where the kept rows span the tensor: the projection wrote zeros)
    u[e] = v;
    th[e] = a.params[e] + rate * v;
  }
}

// grid (nchunks, R), 256 threads
__global__ __launch_bounds__(256) void nsgd_memory_kernel(ultr_dbgd_args a, ultr_nsgd_args n, NsgdLayout ly) {
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, NR = ly.R + 1;
  const int t = nsgd_tensor(ly, c);
  const int64_t base = ly.off[t] + (int64_t)(c - ly.c0[t]) * NSGD_CHUNK, P = ly.P;
  const int len = nsgd_chunk_len(ly, t, base);
  bool lost;
  if (a.need_interleave) {  // no list's winners credit ranker r + 1
    int won = 0;
    for (int b = tid; b < a.batch; b += 256) won |= a.winners[(int64_t)b * NR + r + 1] != 0.f;
    lost = !__syncthreads_or(won);
  } else {  // dbgd_grad_kernel's batch-level winners, summed in its order
    float sg = 0.f, sw = 0.f;
    for (int k = 0; k < NR; ++k) sg += ceilf(a.ndcg[k] - a.ndcg[0]);
    for (int k = 0; k < NR; ++k) sw += ceilf(a.ndcg[k] - a.ndcg[0]) / (sg + 1e-9f);
    lost = sw == 0.f;
  }
  if (tid < len) {
    const int64_t e = (int64_t)r * P + base + tid;
    n.memory[e] = lost ? a.noise[e] : 0.f;
  }
}

static bool nsgd_layout(const ultr_dnn_desc* desc, int R, int64_t n_params, NsgdLayout* ly) {
  DnnPlan p;
  if (!desc || R < 1 || R > NSGD_MAX_R || !ultr_make_dnn_plan(desc, 0, &p)) return false;
  if (n_params >= 0 && p.P != n_params) return false;
  memset(ly, 0, sizeof(*ly));
  ly->nl = p.nl;
  ly->nt = 2 * p.nl;
  ly->R = R;
  ly->np = R * (R + 1) / 2 + R * R;
  ly->P = p.P;
  int64_t chunks = 0;
  for (int j = 0; j < p.nl; ++j) {
    if (p.off_lnb[j] != p.off_lnw[j] + p.K[j] || p.off_b[j] != p.off_w[j] + (int64_t)p.M[j] * p.K[j]) return false;
    ly->K[j] = p.K[j];
    ly->off_ln[j] = p.off_lnw[j];
    ly->off[2 * j] = p.off_w[j];
    ly->len[2 * j] = (int64_t)p.M[j] * p.K[j];
    ly->off[2 * j + 1] = p.off_b[j];
    ly->len[2 * j + 1] = p.M[j];
  }
  for (int t = 0; t < ly->nt; ++t) {
    if (ly->len[t] <= 0 || ly->off[t] + ly->len[t] > ly->P) return false;
    ly->c0[t] = (int)chunks;
    chunks += (ly->len[t] + NSGD_CHUNK - 1) / NSGD_CHUNK;
    if (chunks >= ((int64_t)1 << 30)) return false;
  }
  ly->c0[ly->nt] = ly->nchunks = (int)chunks;
  ly->ws_coef = chunks * ly->np;
  ly->ws_flag = ly->ws_coef + (int64_t)ly->nt * R * R;
  ly->ws_ss = ly->ws_flag + ly->nt;
  return true;
}

static int64_t nsgd_ws_doubles(const NsgdLayout& ly) { return ly.ws_ss + (int64_t)ly.nchunks * ly.R; }

extern "C" int64_t ultr_nsgd_workspace_bytes(const ultr_dnn_desc* desc, int32_t n_rankers) {
  NsgdLayout ly;
  if (!nsgd_layout(desc, n_rankers, -1, &ly)) return -1;
  return 8 * nsgd_ws_doubles(ly);
}

static bool nsgd_args_ok(const ultr_nsgd_args* n, NsgdLayout* ly) {
  if (!n || !n->dbgd || !n->memory) return false;
  const ultr_dbgd_args* a = n->dbgd;
  return dbgd_shape_ok(a) && a->noise && (a->cand_stride == 0 || a->cand_stride >= a->n_params) &&
         nsgd_layout(a->desc, a->n_rankers, a->n_params, ly);
}

extern "C" int ultr_nsgd_noise_args(const ultr_nsgd_args* n, void* stream) {
  NsgdLayout ly;
  if (!nsgd_args_ok(n, &ly) || !n->dbgd->params || !n->dbgd->cand_params || (!n->unit_noise_in && !n->ws)) return ULTR_E_BADARG;
  if (n->ws && ((uintptr_t)n->ws & 7u)) return ULTR_E_BADARG;
  const ultr_dbgd_args a = *n->dbgd;
  const hipStream_t st = (hipStream_t)stream;
  if (!n->unit_noise_in) {
    hipLaunchKernelGGL(nsgd_dot_kernel, dim3(ly.nchunks), dim3(256), 0, st, a, *n, ly);
    hipLaunchKernelGGL(nsgd_solve_kernel, dim3(ly.nt), dim3(1024), 0, st, *n, ly);
    hipLaunchKernelGGL(nsgd_project_kernel, dim3(ly.nchunks), dim3(256), 0, st, a, *n, ly);
  }
  hipLaunchKernelGGL(nsgd_finish_kernel, dim3(ly.nchunks + ly.nl, ly.R), dim3(256), 0, st, a, *n, ly);
  return (int)hipGetLastError();
}

extern "C" int ultr_nsgd_memory_args(const ultr_nsgd_args* n, void* stream) {
  NsgdLayout ly;
  if (!nsgd_args_ok(n, &ly) || (n->dbgd->need_interleave ? !n->dbgd->winners : !n->dbgd->ndcg)) return ULTR_E_BADARG;
  hipLaunchKernelGGL(nsgd_memory_kernel, dim3(ly.nchunks, ly.R), dim3(256), 0, (hipStream_t)stream, *n->dbgd, *n, ly);
  return (int)hipGetLastError();
}
