// ultr_eval.hip — a whole validation / test set evaluated from the dataset RESIDENT in HBM (ResidentDataset), without returning to the
// host between batches (reference main.py:85-227 validate loop, :230-292 test loop; direct_label_feed.py:36-47; data_utils.py:501-514).
//
// The driver walks the set through DirectLabelFeed.get_next_batch: per batch a Python loop that re-assembles the feature rows, a
// staging copy, one validation() call and one host read of its report, then utils.merge_Summary over the per-batch dicts.  Here a chunk of
// `batch` queries is three launches on one stream and the host reads ONE report at the end:
//   eval_pick_kernel        the sequential sibling of online_pick_kernel: queries start .. start + batch - 1, their first list_size
//                           candidates as global document ids [L, B] (PAD = n_docs) and labels [L, B] (0 at a PAD) - what
//                           DirectLabelFeed.prepare_true_labels_with_index builds, with the resident feature matrix in place of the
//                           batch-local copy of the rows;
//   ultr_dnn_forward_metrics the launches validation() issues for that batch (same kernels, same geometry: the same bits);
//   eval_accumulate_kernel  utils.merge_Summary operation for operation in double: acc[i] += (double)mean_i * batch, acc[n] += batch;
//                           the chunk that finishes divides and writes the report into host-mapped memory, the sequence word last.
// No atomics, no reduction across threads: a set's figures are a pure function of (parameters, dataset, batch).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"

// one workgroup of 256 threads = four batch slots (one wavefront each); lanes stride the positions: the row read is coalesced along the
// position, the writes are position-major (stride B between lanes, as online_pick_kernel's)
__global__ __launch_bounds__(256) void eval_pick_kernel(const int32_t* __restrict__ lists, const float* __restrict__ labels, int lmax,
                                                        int32_t pad, int64_t start, int B, int L, int32_t* __restrict__ docids_out,
                                                        float* __restrict__ labels_out, int32_t* __restrict__ query_idx_out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t q = start + b;  // (< n_queries: checked by the host)
  const int32_t* row = lists + q * lmax;
  const float* lab = labels + q * lmax;
  for (int l = lane; l < L; l += 64) {
    const int32_t d = l < lmax ? row[l] : -1;
    int32_t id = pad;
    float y = 0.f;
    if (d >= 0) {
      id = d;
      y = lab[l];
    }
    docids_out[(int64_t)l * B + b] = id;
    labels_out[(int64_t)l * B + b] = y;
  }
  if (lane == 0 && query_idx_out != nullptr) query_idx_out[b] = (int32_t)q;
}

extern "C" int ultr_eval_pick(const int32_t* lists, const float* labels, int64_t n_queries, int32_t lmax, int64_t n_docs, int64_t start,
                              int32_t batch, int32_t list_size, int32_t* docids_out, float* labels_out, int32_t* query_idx_out,
                              void* stream) {
  if (!lists || !labels || !docids_out || !labels_out || n_queries <= 0 || lmax <= 0 || n_docs < 0 || n_docs >= ((int64_t)1 << 31) ||
      start < 0 || batch <= 0 || start > n_queries - batch || list_size <= 0)
    return ULTR_E_BADARG;
  hipLaunchKernelGGL(eval_pick_kernel, dim3((batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, lists, labels, (int)lmax, (int32_t)n_docs,
                     start, (int)batch, (int)list_size, docids_out, labels_out, query_idx_out);
  return (int)hipGetLastError();
}

#define EVAL_MAX_VALUES 128                       // ULTR_MAX_METRICS x 16 cutoffs
#define EVAL_COUNT_SLOT EVAL_MAX_VALUES           // host_report[128]: the summed weights
#define EVAL_SEQ_WORD (2 * (EVAL_MAX_VALUES + 1))  // the report's sequence word (32-bit index): behind 129 doubles

// ONE workgroup, thread i owns value i: merge_Summary's `total[k] = total.get(k, 0.0) + v * w`, `wsum[k] += w` and, at the end,
// `total[k] / max(0.0000001, wsum[k])` in Python's own (double) arithmetic.  v is a float32 and w a batch size: v * w is exact in
// double below 2^29 lists per batch, so contracting the multiply-add changes nothing; the division is IEEE round-to-nearest.
__global__ __launch_bounds__(EVAL_MAX_VALUES) void eval_accumulate_kernel(const float* __restrict__ means, int n, int batch,
                                                                          double* __restrict__ acc, int flags,
                                                                          double* __restrict__ host, uint32_t seq) {
  __shared__ double sm_wsum;
  const int i = threadIdx.x;
  const bool finish = (flags & ULTR_EVAL_FINISH) != 0;
  const double w = (double)batch;
  double a = 0.0;
  if (i < n) {
    a = (flags & ULTR_EVAL_RESET) ? 0.0 : acc[i];
    a = __dadd_rn(a, __dmul_rn((double)means[i], w));
    acc[i] = a;
  }
  if (i == 0) {  // (thread 0 owns a value AND the weight sum: n may be the whole workgroup)
    double ws = (flags & ULTR_EVAL_RESET) ? 0.0 : acc[n];
    ws = __dadd_rn(ws, w);
    acc[n] = ws;
    sm_wsum = ws;
  }
  if (!finish) return;
  __syncthreads();
  const double wsum = sm_wsum;
  if (i < n) __hip_atomic_store(host + i, __ddiv_rn(a, fmax(1e-7, wsum)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (i == 0) __hip_atomic_store(host + EVAL_COUNT_SLOT, wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // the report's values have left every wave before the sequence word follows them (ultr_metrics_report's order: values, wait, word)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (i == 0) __hip_atomic_store(reinterpret_cast<uint32_t*>(host) + EVAL_SEQ_WORD, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" int ultr_eval_accumulate(const float* batch_means, int32_t n_values, int32_t batch, double* acc, int32_t flags,
                                    double* host_report, uint32_t seq, void* stream) {
  if (!batch_means || !acc || n_values <= 0 || n_values > EVAL_MAX_VALUES || batch <= 0 ||
      (flags & ~(ULTR_EVAL_RESET | ULTR_EVAL_FINISH)) != 0 || ((flags & ULTR_EVAL_FINISH) && !host_report))
    return ULTR_E_BADARG;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(EVAL_MAX_VALUES), 0, (hipStream_t)stream, batch_means, (int)n_values, (int)batch,
                     acc, (int)flags, host_report, seq);
  return (int)hipGetLastError();
}

// The whole set from ONE host call: per chunk of `batch` queries (the last one short) the pick, validation()'s own forward + metric
// launch (its host report NULL) and the accumulate - reset on the first chunk, finish on the last.  Chunking by `batch` is deliberate:
// the launches are exactly the ones the per-batch loop issues, so the merged figures are the driver's, not merely close to them.
extern "C" int ultr_dnn_eval_set(const ultr_dnn_desc* d, const float* params, const float* wt, const float* features, int64_t n_docs,
                                 const int32_t* lists, const float* labels, int64_t n_queries, int32_t lmax, int32_t batch,
                                 int32_t list_size, const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics,
                                 float max_label, int32_t* docids_ws, float* labels_ws, float* scores_ws, float* out, int32_t* order_out,
                                 float* masked_out, float* ws, uint32_t* counter, float* scores_all, float* per_query, double* acc,
                                 double* host_report, uint32_t seq, void* stream) {
  if (!docids_ws || !labels_ws || !scores_ws || !out || !ws || !counter || !acc || !host_report || n_queries <= 0 || batch <= 0 || list_size <= 0 ||
      n_topn <= 0 || n_topn > 16 || n_metrics <= 0 || n_metrics > ULTR_MAX_METRICS)
    return ULTR_E_BADARG;
  const int32_t width = n_metrics * n_topn;  // <= EVAL_MAX_VALUES
  for (int64_t start = 0; start < n_queries; start += batch) {
    const int32_t b = (int32_t)(n_queries - start < batch ? n_queries - start : batch);
    int rc = ultr_eval_pick(lists, labels, n_queries, lmax, n_docs, start, b, list_size, docids_ws, labels_ws, nullptr, stream);
    if (rc != 0) return rc;
    float* sc = scores_all != nullptr ? scores_all + start * list_size : scores_ws;
    float* pq = per_query != nullptr ? per_query + start * width : ws;
    rc = ultr_dnn_forward_metrics(d, params, wt, features, n_docs, docids_ws, labels_ws, b, list_size, sc, topn, n_topn, metric_ids,
                                  n_metrics, max_label, out, order_out, masked_out, pq, counter, nullptr, 0u, stream);
    if (rc != 0) return rc;
    const int32_t flags = (start == 0 ? ULTR_EVAL_RESET : 0) | (start + b >= n_queries ? ULTR_EVAL_FINISH : 0);
    rc = ultr_eval_accumulate(out, width, b, acc, flags, host_report, seq, stream);
    if (rc != 0) return rc;
  }
  return 0;
}
