// ultr_feed.h - the click draw of ultr_feed.hip as a device function: its own launch (click_batch_kernel) or a rider on the update
// launch of the step in front of it (update_tiled_kernel: extra workgroups behind the update's own - ultr_feed_train_step).  The
// click model, its decisions and the walk over a list are ultr_click.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_click.h"
#include "ultr_device.h"

// Philox counter word 3 of the draws that share click_draw's key: the query pick, the click uniforms, and the per-session shuffle keys
// of the propensity estimator (ultr_propensity.hip)
#define ULTR_QUERY_TAG 0x51ED270Bu
#define ULTR_CLICK_TAG 0x2545F491u
#define ULTR_SHUFFLE_TAG 0x53485546u

// one workgroup of 256 threads = four batch slots (one per wave); `block` = the workgroup's index among the draw's (batch + 3) / 4
__device__ __forceinline__ void click_draw(const ultr_click_args& ca, int block) {
  const int32_t* __restrict__ lists = ca.lists;
  const float* __restrict__ rel = ca.labels;
  const int64_t n_queries = ca.n_queries, n_docs = ca.n_docs;
  const int Lmax = ca.lmax, B = ca.batch, L = ca.list_size, max_tries = ca.max_tries;
  const ClickModel cm = click_model_of(ca);
  int32_t* __restrict__ docids = ca.docids;
  float* __restrict__ clicks = ca.clicks;
  int32_t* __restrict__ qidx = ca.query_idx;
  const int lane = threadIdx.x & 63;
  const int b = block * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const Philox rng = philox_step_key(ca.seed, ca.step);
  int64_t q = 0;
  for (int attempt = 0; attempt < max_tries; ++attempt) {
    uint32_t c[4] = {(uint32_t)b, (uint32_t)attempt, 0xFFFFFFFFu, ULTR_QUERY_TAG};
    rng(c);
    q = (int64_t)((double)u01(c[0]) * (double)n_queries);  // uniform query pick (click_simulation_feed.py:126)
    if (q >= n_queries) q = n_queries - 1;
    int32_t id = (int32_t)n_docs;  // the document of this lane's position: gathered with its label, written with its click
    const float any = wave_click_walk(
        cm, rng, (uint32_t)b, (uint32_t)attempt, ULTR_CLICK_TAG, L, lane,
        [&](int l) {
          const int32_t d = (l < Lmax) ? lists[q * Lmax + l] : -1;
          // a PAD position counts as a label-0 document and CAN be clicked, exactly as in the reference feed
          // (click_simulation_feed.py:74-81 builds the label list with 0 for pads and samples every position)
          float y = 0.f;
          id = (int32_t)n_docs;
          if (d >= 0) {
            id = d;
            y = rel[q * Lmax + l];
          }
          return y;
        },
        [&](int l, float ck) {
          docids[(int64_t)l * B + b] = id;
          clicks[(int64_t)l * B + b] = ck;
        });
    if (any > 0.f) break;  // lists without a click are rejected (click_simulation_feed.py:89-91)
  }
  if (lane == 0 && qidx != nullptr) qidx[b] = (int32_t)q;
}

inline bool ultr_click_args_ok(const ultr_click_args* c) {
  return c && c->lists && c->labels && c->docids && c->clicks && c->n_queries > 0 && c->lmax > 0 && c->batch > 0 && c->list_size > 0 &&
         c->max_tries > 0 && c->n_docs >= 0 && c->n_docs < ((int64_t)1 << 31) && click_model_ok(click_model_of(*c));
}
