// ultr_step.hip — one host call per training step: forward -> loss -> backward -> (update).
// Exists to keep the HOST out of the critical path: at ~100 us of GPU work per step, four separate FFI calls from
// Python (argument marshalling + launches) cost more than a third of that.  No new device code here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ultr_hip.h"
#include "ultr_listloss.h"
#include "ultr_plan.h"
#include "ultr_prof.h"

// behind the backward: (data parallel) the one-kernel exchange of grads[P + tail] with its sum-of-squares partials, then the
// update - or stop for the caller (skip_update: it runs a process-group all-reduce + ultr_grad_sumsq + ultr_apply_update)
static int finish_step(const ultr_step_args* a, StepCtx* ctx, void* stream) {
  if (a->comm != nullptr && !a->skip_update) {
    const int64_t P = ultr_dnn_param_count(a->desc);
    if (P <= 0) return ULTR_E_BADARG;
    const int64_t n = P + ultr_tail_len(a->list_size);
    if (!ctx->xchg_done) {  // (the slab reduction of this step's backward did not run the exchange itself)
      // (early_dp.host is null when the weight-gradient launch of this step already exchanged the head of the tail and reported the loss)
      const int rc = ultr_comm_allreduce_ex(a->comm, a->comm_step, a->grads, n, P, a->grads, a->bwd_ws, (int32_t)((n + 63) / 64), stream,
                                            ctx->early_dp);
      if (rc) return rc;
    }
    // the update behind the exchange is guarded by the communicator's status word: after a timed-out peer wait (here or on
    // any peer - the rank that times out raises the word everywhere) no replica moves its parameters again
    ultr_update_desc u = *a->upd;
    u.guard = ultr_comm_status_word(a->comm);
    // (level-2 partials: only when the slab-reduction launch exchanged the vector itself - the stand-alone exchange kernel writes level 1)
    return ultr_apply_update_ex(&u, a->desc, a->params, a->wt, a->state, a->grads, a->aux, a->bwd_ws, a->scalars,
                                ctx->xchg_done ? ctx->nsq2 : 0, &ctx->rider, stream);
  } else if (a->skip_update) {
    return 0;
  }
  return ultr_apply_update_ex(a->upd, a->desc, a->params, a->wt, a->state, a->grads, a->aux, a->bwd_ws, a->scalars, ctx->nsq2, &ctx->rider,
                              stream);
}

extern "C" int ultr_train_step(const ultr_step_args* a, void* stream) {
  StepCtx ctx;
  return ultr_train_step_ctx(a, &ctx, stream);
}

int ultr_train_step_ctx(const ultr_step_args* a, StepCtx* ctx, void* stream) {
  if (!a || !a->desc || !a->upd) return ULTR_E_BADARG;
  // the update launch would refuse these behind the backward: refuse them here, with nothing launched
  if (!a->skip_update && ultr_update_check_opt(a->upd, a->state)) return ULTR_E_BADARG;
  // the step keeps the weight copies current (its update launch writes them with 16-byte stores): one off a 16-byte boundary is
  // refused; an absent one is fine - every stage then streams the row-major parameters (the operand contract, ultr_plan.h)
  if (!ultr_aligned16(a->wt)) return ULTR_E_BADARG;
  ultr_prof_tick();
  // early loss report of this step's backward (EarlyReport, ultr_plan.h): only where the reported loss has no L2 term (that one is
  // formed by the update launch) - from the local loss sums where they ARE the batch's, behind the peer exchange in a data-parallel step
  const ultr_update_desc* u = a->upd;
  const bool dp = a->comm != nullptr && !a->skip_update;
  const bool ok = u->host_scalars != nullptr && a->comm == nullptr && !a->skip_update && u->l2_loss == 0.f;
  const bool early_dp = dp && u->host_scalars != nullptr && u->l2_loss == 0.f;
  ctx->wt = a->wt;
  ctx->early = {ok ? u->host_scalars : nullptr, u->seq, u->algo, u->ranker_loss_weight};
  ctx->comm = dp ? a->comm : nullptr;
  ctx->comm_step = a->comm_step;
  ctx->early_dp = {early_dp ? u->host_scalars : nullptr, u->seq, u->algo, u->ranker_loss_weight};
  // pair-walk losses: the short kernel for every list it takes, the long one only for a list it refuses (loss_route,
  // ultr_listloss.h) - decided here, so that a list neither takes is refused before the forward is launched
  const int route = loss_route(a->upd->algo, a->list_size);
  if (route < 0) return route;
  // AffineRank's table [alpha(n) | beta(n)] rides in ipw_table: a missing one is refused here too, with nothing launched
  if (a->upd->algo == ULTR_ALGO_AFFINE && (!a->ipw_table || a->n_ipw <= 0)) return ULTR_E_BADARG;
  const bool long_list = route == LOSS_ROUTE_LONG;
  int rc;
  if (a->upd->algo == ULTR_ALGO_SOFTMAX) {
    // small batches (NA / IPW): forward + loss + backward as ONE launch when the shape qualifies
    rc = ultr_fused_step_softmax(a->desc, a->params, a->wt, a->features, a->n_docs, a->docids, a->batch, a->list_size,
                                 a->scores, a->saved, a->labels, a->pw, a->ipw_table, a->n_ipw, a->dscores, a->loss_ws,
                                 a->bwd_ws, a->grads, stream, ctx);
    if (rc == 0) return finish_step(a, ctx, stream);
    if (rc != ULTR_E_UNSUPPORTED) return rc;
  }
  rc = ultr_dnn_forward(a->desc, a->params, a->wt, a->features, a->n_docs, a->docids, a->batch, a->list_size,
                            a->scores, a->saved, stream);
  if (rc) return rc;
  if (a->upd->algo == ULTR_ALGO_SOFTMAX) {
    // NA / IPW: the loss is fused into the backward kernel's prologue (one launch and one dependent kernel
    // boundary fewer); ultr_softmax_ce stays available as the stand-alone stage
    rc = ultr_dnn_backward_softmax_ctx(a->desc, a->params, a->features, a->n_docs, a->docids, a->batch, a->list_size, a->saved,
                                       a->scores, a->labels, a->pw, a->ipw_table, a->n_ipw, a->dscores, a->loss_ws, a->bwd_ws,
                                       a->grads, stream, ctx);
    if (rc) return rc;
    return finish_step(a, ctx, stream);
  }
  switch (a->upd->algo) {
    case ULTR_ALGO_DLA:
      rc = ultr_dla_loss(a->scores, a->labels, a->aux, a->upd->logits_to_prob, a->batch, a->list_size, a->dscores,
                         a->loss_ws, stream);
      break;
    case ULTR_ALGO_PAIRDEBIAS:
      rc = (long_list ? ultr_pairdebias_loss_long : ultr_pairdebias_loss)(
          a->scores, a->labels, a->aux, a->aux ? a->aux + a->list_size : nullptr, a->batch, a->list_size,
          a->batch_total > 0 ? a->batch_total : a->batch, a->dscores, a->loss_ws, stream);
      break;
    case ULTR_ALGO_LAMBDARANK:
      rc = (long_list ? ultr_lambdarank_loss_long : ultr_lambdarank_loss)(
          a->scores, a->labels, a->aux, a->aux ? a->aux + a->list_size : nullptr, a->sigma, a->batch, a->list_size, a->dscores,
          a->loss_ws, stream);
      break;
    case ULTR_ALGO_PRS:
      // pw: a weight per list entry (an estimator that reads the list's clicks) instead of the position table
      rc = a->pw != nullptr
               ? (long_list ? ultr_prs_loss_pw_long : ultr_prs_loss_pw)(a->scores, a->labels, a->pw, a->sigma, a->batch, a->list_size,
                                                                        a->dscores, a->loss_ws, stream)
               : (long_list ? ultr_prs_loss_long : ultr_prs_loss)(a->scores, a->labels, a->ipw_table, a->n_ipw, a->sigma, a->batch,
                                                                  a->list_size, a->dscores, a->loss_ws, stream);
      break;
    case ULTR_ALGO_PDGD:
      rc = ultr_pdgd_loss(a->scores, a->labels, a->docids, a->n_docs, a->sigma, a->n_ipw, a->batch, a->list_size, a->dscores,
                          a->loss_ws, stream);
      break;
    case ULTR_ALGO_REGEM:
      rc = ultr_regem_loss(a->scores, a->labels, a->aux, a->uniforms, a->rng_seed, a->rng_step, a->batch, a->list_size,
                           a->dscores, nullptr, a->loss_ws, stream);
      break;
    case ULTR_ALGO_TWOTOWER:  // the combination and the mask flag travel in logits_to_prob (include/ultr_hip.h)
      rc = ultr_twotower_loss(a->scores, a->labels, a->aux, a->upd->logits_to_prob & ULTR_TWOTOWER_SUM,
                              (a->upd->logits_to_prob & ULTR_TWOTOWER_MASK) ? a->docids : nullptr, a->n_docs, a->batch, a->list_size,
                              a->dscores, a->loss_ws, stream);
      break;
    case ULTR_ALGO_PLRANK: {  // cutoff, sample count and gain travel in logits_to_prob (ULTR_PLRANK_PACK, include/ultr_hip.h)
      const int32_t pk = a->upd->logits_to_prob;
      rc = ultr_plrank_loss(a->scores, a->labels, a->pw, a->ipw_table, a->n_ipw, a->docids, a->n_docs, pk & 0xFFF, (pk >> 12) & 0xFFF,
                            (pk >> 24) & 1, a->rng_seed, a->rng_step, a->batch, a->list_size, a->dscores, nullptr, a->loss_ws, stream);
      break;
    }
    case ULTR_ALGO_AFFINE:  // ipw_table = [alpha(n) | beta(n)], n_ipw = n; the PAD-mask flag travels in logits_to_prob
      rc = ultr_affine_loss(a->scores, a->labels, a->ipw_table, a->ipw_table + a->n_ipw, a->n_ipw,
                            (a->upd->logits_to_prob & ULTR_AFFINE_MASK) ? a->docids : nullptr, a->n_docs, a->batch, a->list_size,
                            a->dscores, a->loss_ws, stream);
      break;
    default:
      return ULTR_E_BADARG;
  }
  if (rc) return rc;
  rc = ultr_dnn_backward_ctx(a->desc, a->params, a->features, a->n_docs, a->docids, a->batch, a->list_size, a->saved,
                             a->dscores, a->loss_ws, a->bwd_ws, a->grads, stream, ctx);
  if (rc) return rc;
  return finish_step(a, ctx, stream);
}
