/*
 * ultr_hip.h — C ABI of libultr_hip.so, the MI355X (gfx950) hot path of the unbiased
 * learning-to-rank engine.
 *
 * This is the drop-in boundary.  Every entry point replaces one stretch of the
 * reference's (ULTR-Community/ULTRA_pytorch) pure-PyTorch hot path; the reference
 * file:line each one stands in for is cited on the declaration.  The Python plugin
 * classes in ultra_pytorch_amd/ (same constructor / train / validation / build
 * contracts as ultra.learning_algorithm.* and ultra.ranking_model.DNN) bind these
 * symbols with ctypes — see INTEGRATION.md for the stub a reference maintainer adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  No torch types.
 *   - ALL data pointers are DEVICE pointers owned by the caller, fp32 unless noted.
 *   - Every function enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns immediately: 0 on success, a hipError_t value (>0) on a HIP failure,
 *     or a negative ULTR_E_* code for a bad argument.  Nothing throws, nothing syncs,
 *     nothing allocates: scratch comes from caller-provided workspaces sized by the
 *     ultr_*_workspace_bytes() queries (host-only arithmetic, callable without a GPU).
 *   - Layouts follow the reference's feed (click_simulation_feed.py:141-156):
 *       features  [n_docs, F]   row-major; the PAD document has id == n_docs and is an
 *                               all-zero row that is NOT stored (base_algorithm.py:148-149)
 *       docids    [L, B] int32  position-major (docid_input{l}[b])
 *       labels    [L, B]        position-major (label{l}[b]) — clicks or relevance
 *       scores    [B, L]        list-major, what BaseAlgorithm.ranking_model returns
 *                               (base_algorithm.py:118-132)
 *     Internally a "row" is one (query, position) document: row n = b*L + l.
 *   - Parameters travel as ONE flat fp32 vector in the reference's state_dict order
 *     (DNN.py:41-55): for j = 0..k:  layer_norm{j}.weight[K_j], layer_norm{j}.bias[K_j],
 *     linear{j}.weight[M_j,K_j] row-major, linear{j}.bias[M_j]; K_0 = F, M_k = 1.
 */
#ifndef ULTR_HIP_H
#define ULTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ULTR_ABI_VERSION 8
#define ULTR_MAX_HIDDEN 7 /* hidden layers; Linear layers = hidden + 1 <= 8 */

#define ULTR_E_BADARG (-1)
#define ULTR_E_UNSUPPORTED (-2)
#define ULTR_E_WORKSPACE (-3)
#define ULTR_E_COMM_TIMEOUT (-4) /* a peer did not arrive within the bounded wait of ultr_comm_allreduce */
/* bit of the status word of the step report (ultr_update_desc::host_scalars[8]) that is NOT a communication failure: a hidden
 * weight reached |w| >= 128, outside the range of the split-half (fp16 hi / lo, x 2^8) weight copies the wide layers' products
 * read - results from then on are not to be trusted; run with ULTR_FB_H3=0 ULTR_FWD_H3=0 ULTR_BWD_H3=0 (fp32 matrix-core
 * products).  Raised by ultr_dnn_build_wt / ultr_apply_update, reported with the step after the one that wrote the weight. */
#define ULTR_STATUS_H3_RANGE 0x100u
/* ... and the early warning: a hidden weight reached |w| >= 64, half of that range, while every copy is still exact.  An optimizer
 * step moves a weight by at most learning_rate x max_gradient_norm, so a host that reads the report every few steps has time to
 * switch THIS model to the fp32 products (ultr_dnn_desc::flags |= ULTR_MODEL_FP32_PRODUCTS) before anything overflows - engine.StepEngine does, with a
 * warning: like the reference (base_algorithm.py:208-226) the library then trains any weight magnitude. */
#define ULTR_STATUS_H3_NEAR 0x200u
/* bits of a range-flag word (ultr_update_desc::range_flag, the word inside `wt`): a scaled weight overflowed / is near the edge */
#define ULTR_H3_FLAG_OVER 1u
#define ULTR_H3_FLAG_NEAR 2u

/* base_ranking_model.py:63-69 (ACT_FUNC_DIC): elu, relu, tanh, sigmoid.  ('selu' is listed there as a plain function and
 * nn.Sequential.add_module rejects it - TypeError at DNN.py:52-53 - so it is not an option of the reference.) */
enum ultr_activation { ULTR_ACT_ELU = 0, ULTR_ACT_RELU = 1, ULTR_ACT_TANH = 2, ULTR_ACT_SIGMOID = 3 };

/* DNN.__init__ hyper-parameters (DNN.py:25-38).  norm is always 'layer'
 * (LayerNorm before EVERY Linear, DNN.py:43-47). */
typedef struct ultr_dnn_desc {
  int32_t feature_size;            /* F = K_0 */
  int32_t n_hidden;                /* k; 0 reproduces ultra.ranking_model.Linear */
  int32_t hidden[ULTR_MAX_HIDDEN]; /* hidden_layer_sizes */
  int32_t activation;              /* ultr_activation */
  /* ABI 6: per-MODEL switches (0 = defaults).  ULTR_MODEL_FP32_PRODUCTS: every product of this model on the fp32 matrix cores
   * (v_mfma_f32_16x16x4_f32), whatever the process-wide ULTR_*_H3 knobs say - what a caller sets when a hidden weight of THIS
   * model approaches the range of the split-half weight copies (ULTR_STATUS_H3_NEAR); other models of the process keep their plan. */
  int32_t flags;
} ultr_dnn_desc;
#define ULTR_MODEL_FP32_PRODUCTS 1
/* ultr_setrank_desc::flags only: train this SetRank model at any list size.  Where the one-pass attention backward refuses (beyond 128
 * documents on the matrix cores, 120 on the scalar kernel; and from ULTR_SR_ATTN_LONG_MIN on) the backward streams partner tiles through
 * LDS, and the FORWARD streams at the same list sizes - the streaming backward reads the forward's row statistic, which the one-pass
 * scalar forward of 129 .. 256 documents does not write.  That range is the one place where the scores of a model with the flag differ
 * in bits from one without; below the hand-over both run the one-pass kernels.  ultr_setrank_workspace_bytes grows by
 * n_rows x num_heads floats for such a descriptor. */
#define ULTR_MODEL_SR_STREAM_BWD 2

/* ---- host-only queries ------------------------------------------------------------- */
int ultr_abi_version(void);
/* number of fp32 parameters P (0 on bad desc) */
int64_t ultr_dnn_param_count(const ultr_dnn_desc* d);
/* offsets[4*(k+1)] of ln.weight, ln.bias, linear.weight, linear.bias per layer */
int ultr_dnn_param_offsets(const ultr_dnn_desc* d, int64_t* offsets);
/* bytes of `saved` (activations + LayerNorm statistics kept by a training forward) */
int64_t ultr_dnn_saved_bytes(const ultr_dnn_desc* d, int64_t n_rows);
/* bytes of `bwd_ws` (dz buffers + deterministic partial-sum slabs) */
int64_t ultr_dnn_bwd_workspace_bytes(const ultr_dnn_desc* d, int64_t n_rows);
/* floats in the step vector that follows the P gradients in `grads` (see ultr_dnn_backward) */
int64_t ultr_step_tail_floats(int32_t list_size);
/* bytes of `loss_ws` for B lists of size L */
int64_t ultr_loss_workspace_bytes(int64_t batch, int32_t list_size);
/* step-tail partials the stand-alone ultr_*_loss kernels leave in `loss_ws` (one per workgroup) = the n_loss_parts of
 * ultr_setrank_backward */
int64_t ultr_loss_part_count(int64_t batch);
/* Dynamic LDS in bytes that the stand-alone loss kernel of `algo` (ULTR_ALGO_SOFTMAX .. ULTR_ALGO_PDGD, ULTR_ALGO_TWOTOWER,
 * ULTR_ALGO_PLRANK, ULTR_ALGO_AFFINE) requests at list_size
 * (additive within ABI 8; host-only, launches nothing) - read from the layout the kernel itself carves its LDS with
 * (csrc/ultr_listloss.h).  ULTR_E_UNSUPPORTED where the entry would refuse the list size: beyond 64 KiB for ultr_softmax_ce,
 * ultr_affine_loss, ultr_dla_loss, ultr_regem_loss and ultr_twotower_loss, beyond 160 KiB for ultr_pairdebias_loss, ultr_lambdarank_loss, ultr_prs_loss
 * and ultr_plrank_loss, beyond 256
 * documents for ultr_pdgd_loss - the longest accepted lists are stated with each entry below.  ULTR_E_BADARG: an algorithm without a
 * stand-alone loss kernel, list_size <= 0. */
int64_t ultr_loss_lds_bytes(int32_t algo, int32_t list_size);

/* ---- a2 + a3: gather + DNN forward --------------------------------------------------
 * Replaces BaseAlgorithm.get_ranking_scores + ranking_model (base_algorithm.py:118-154)
 * and DNN.build (DNN.py:58-88): np.take of feature rows (zero PAD row for id == n_docs),
 * then [LayerNorm -> Linear -> act] x k -> LayerNorm -> Linear(.,1), scores as [B, L].
 * saved == NULL: inference (validation) forward; otherwise activations and LayerNorm
 * statistics are kept for ultr_dnn_backward.
 * The operand contract (one rule for every DNN entry point; ultr_dnn_route_operands answers for it):
 *   params, features: any 4-byte aligned address (a slice of a larger buffer, a candidate vector at any stride).  On a 16-byte
 *     boundary the kernels take float4 loads, off it the scalar builds of the same kernels; the results agree to rounding.
 *   wt: NULL, or the buffer ultr_dnn_build_wt filled.  Every kernel that reads it uses 16-byte loads, so a copy that is NOT on a
 *     16-byte boundary counts as ABSENT wherever it is only read: here, in ultr_dnn_forward_ndcg / _metrics and in the backward
 *     stages of ultr_train_step.  The calls that must WRITE it - ultr_apply_update, ultr_train_step - refuse it with
 *     ULTR_E_BADARG before anything is launched.  wt == NULL is accepted everywhere: the generic kernels read W directly.
 *   the other buffers (scores, saved, dscores, workspaces, grads) are the library's own sizes at allocator alignment (16 bytes). */
int ultr_dnn_forward(const ultr_dnn_desc* d, const float* params, const float* wt, const float* features,
                     int64_t n_docs, const int32_t* docids, int32_t batch, int32_t list_size, float* scores,
                     void* saved, void* stream);

/* k-major copy of the hidden Linear weights (WT_j = W_j^T): lets the forward stream MFMA B-fragments as
 * 256-byte contiguous pieces.  `wt` has ultr_dnn_wt_floats(d) floats; build it once after the parameters
 * were written from outside (load_state_dict / init), ultr_apply_update keeps it current afterwards.
 * Passing wt == NULL to ultr_dnn_forward selects the (slower) generic path that reads W directly. */
int64_t ultr_dnn_wt_floats(const ultr_dnn_desc* d);
int ultr_dnn_build_wt(const ultr_dnn_desc* d, const float* params, float* wt, void* stream);
/* ABI 5.  Range state of the split-half (fp16 hi / lo) weight copies inside `wt` (ULTR_STATUS_H3_NEAR / _RANGE above):
 * 0 = every hidden weight is below 64 in magnitude, 1 = near the edge (|w| >= 64, copies still exact), 2 = a copy overflowed
 * (|w| >= 128).  SYNCHRONISES the stream (one 4-byte device-to-host copy): meant to be called once behind ultr_dnn_build_wt,
 * i.e. after parameters arrived from outside (checkpoint, init) - the reference accepts any weight there (DNN.py:58-88 computes
 * in fp32), so the caller switches to the fp32 products (ULTR_FB_H3=0 ULTR_FWD_H3=0 ULTR_BWD_H3=0 + ultr_config_reload) when
 * this is not 0.  During training the same information arrives with the step report (host_scalars[8]). */
int ultr_dnn_wt_range(const ultr_dnn_desc* d, const float* wt, void* stream);
/* Which kernels a call takes (additive within ABI 8; host-only, launches nothing): the route ultr_dnn_forward, ultr_dnn_backward,
 * ultr_dnn_backward_softmax and the fused step decide once per call - the queries below read the same function - at batch x list_size
 * rows gathered from n_docs documents, under the knobs as last read (ultr_config_reload), for what ultr_train_step and the evaluation
 * always pass: 16-byte aligned pointers, the weight copies present and a dscores buffer (ultr_dnn_route_operands takes these
 * facts as an argument); with the CU count the planners read (256 where no device
 * answers).  ULTR_E_UNSUPPORTED where the call itself would refuse (`out` is filled, the family that refuses is ULTR_DNN_UNSUPPORTED);
 * ULTR_E_BADARG: a bad desc, a NULL out, batch <= 0, list_size <= 0, n_docs < 0 or an unknown `call`. */
enum ultr_dnn_route_call {
  ULTR_DNN_CALL_EVAL = 0,          /* ultr_dnn_forward with saved == NULL */
  ULTR_DNN_CALL_STEP_SOFTMAX = 1,  /* ultr_train_step, algo ULTR_ALGO_SOFTMAX */
  ULTR_DNN_CALL_STEP_DSCORES = 2   /* ultr_train_step of an algorithm whose dscores come from its loss kernel */
};
enum ultr_dnn_family {
  ULTR_DNN_NONE = 0,         /* not part of this call */
  ULTR_DNN_TILE = 1,         /* dnn_fwd_kernel / dnn_bwd_kernel: 16- or 32-row tiles */
  ULTR_DNN_TILE2 = 2,        /* dnn_bwd2_kernel (backward only) */
  ULTR_DNN_WIDE = 3,         /* dnn_fwdw_kernel / dnn_bwdw_kernel: 17 .. 64 rows per workgroup */
  ULTR_DNN_PER_LAYER = 4,    /* the per-layer launches (training forward, backward) */
  ULTR_DNN_FUSED = 5,        /* ran inside dnn_fb_kernel */
  ULTR_DNN_UNSUPPORTED = 6   /* the call returns ULTR_E_UNSUPPORTED */
};
enum ultr_dnn_loss_place {
  ULTR_DNN_LOSS_NONE = 0,      /* evaluation */
  ULTR_DNN_LOSS_LAUNCH = 1,    /* a launch of its own (ultr_softmax_ce, or the algorithm's loss kernel) */
  ULTR_DNN_LOSS_PROLOGUE = 2,  /* the prologue of dnn_bwd_kernel / dnn_bwd2_kernel */
  ULTR_DNN_LOSS_FUSED = 3      /* inside dnn_fb_kernel */
};
typedef struct ultr_dnn_route_info {
  int32_t fused_waves;        /* 0: the separate kernels; 8 / 16: dnn_fb_kernel on that many waves per workgroup */
  int32_t fwd, fwd_rows;      /* ultr_dnn_family of the forward and its rows per workgroup (0: per-layer; dnn_fb_kernel: the live
                               * rows of its 16-row tile, whole lists) */
  int32_t bwd, bwd_rows;      /* ... of the row-local backward */
  int32_t loss;               /* ultr_dnn_loss_place */
  int32_t wg_split_half;      /* 1: the weight gradients take dnn_wgrad_h3_kernel */
  int32_t reserved[5];        /* 0 */
} ultr_dnn_route_info;
int ultr_dnn_route(const ultr_dnn_desc* d, int32_t batch, int32_t list_size, int64_t n_docs, int32_t call, ultr_dnn_route_info* out);
/* The same for any operands (additive within ABI 8): `operands` = the ULTR_DNN_OP_ bits of what the call passes; ultr_dnn_route is
 * ULTR_DNN_OP_ALL.  PARAMS16 / FEATURES16: that pointer is on a 16-byte boundary.  WT: the weight copies are passed; WT16: they are
 * on a 16-byte boundary - by the operand contract (ultr_dnn_forward) a copy off it counts as absent, so clearing either bit gives
 * the same route.  DSCORES: a [B, L] dscores buffer exists (ultr_dnn_backward_softmax's dscores_out, ultr_step_args::dscores);
 * without one the softmax loss runs in the backward kernel's prologue, which the wide-tile and per-layer backward do not have.
 * The public ultr_dnn_backward / ultr_dnn_backward_softmax never see the copies: their route is the step's with WT clear.
 * ULTR_E_BADARG also for a bit outside ULTR_DNN_OP_ALL. */
#define ULTR_DNN_OP_PARAMS16 1u
#define ULTR_DNN_OP_FEATURES16 2u
#define ULTR_DNN_OP_WT 4u
#define ULTR_DNN_OP_WT16 8u
#define ULTR_DNN_OP_DSCORES 16u
#define ULTR_DNN_OP_ALL 31u
int ultr_dnn_route_operands(const ultr_dnn_desc* d, int32_t batch, int32_t list_size, int64_t n_docs, int32_t call, uint32_t operands,
                            ultr_dnn_route_info* out);
/* The older queries, views of the same route (for tests, tools and the bench line).  Which forward kernel ultr_dnn_forward launches
 * for n_rows = batch x list_size rows: 16 / 32 = dnn_fwd_kernel with that many rows per workgroup, 1000 + R = the wide-tile kernel
 * dnn_fwdw_kernel with R = 17 .. 64 rows per workgroup, 0 = the per-layer path (training forward only), < 0 = bad descriptor.
 * They name the kernel that is launched: where nothing can take the float4 paths - a feature or hidden width that is no multiple
 * of 4, ULTR_NO_VEC=1 - that is a 16- / 32-row tile kernel (before the route existed they answered "wide" or "per-layer" there). */
int32_t ultr_dnn_forward_tile_rows(const ultr_dnn_desc* d, int64_t n_rows, int32_t training);
/* ... and the row-local backward kernel of ultr_train_step (dscores from a loss kernel): 16 / 32 = dnn_bwd2_kernel / dnn_bwd_kernel
 * (ultr_dnn_route tells them apart), 1000 + R = the wide-tile kernel dnn_bwdw_kernel, 0 = the per-layer path. */
int32_t ultr_dnn_backward_tile_rows(const ultr_dnn_desc* d, int64_t n_rows);
/* ... and whether a softmax / IPW training step of `batch` lists of `list_size` takes the fused forward + loss + backward kernel
 * dnn_fb_kernel: 0 = no (the separate kernels), 8 / 16 = yes, with that many waves per workgroup (ULTR_FB_NW). */
int32_t ultr_fused_fb_waves(const ultr_dnn_desc* d, int32_t batch, int32_t list_size);

/* ---- a5 (backward half): what loss.backward() does for the DNN ----------------------
 * Replaces autograd through DNN.sequential (called from BaseAlgorithm.opt_step,
 * base_algorithm.py:208-226).  Input dscores[B, L] = d(loss)/d(scores) up to the scalar
 * factor the loss kernels keep separate (see tail).  Output grads[P + tail]: the flat
 * parameter gradient (UNSCALED) followed by the step vector `tail` =
 *   [0] loss_sum  [1] D  [2] loss2_sum  [3] D2  [4..4+2L) per-position sums
 * copied (summed in fixed order) from the loss workspace `loss_ws`.  Per-block partial sums of
 * squares of the P unscaled gradients are left at the head of bwd_ws (single-GPU fast path).
 * The whole buffer grads[0 .. P+tail) is what a data-parallel caller all-reduces; it then calls
 * ultr_grad_sumsq to refresh the partials before ultr_apply_update. */
int ultr_dnn_backward(const ultr_dnn_desc* d, const float* params, const float* features, int64_t n_docs,
                      const int32_t* docids, int32_t batch, int32_t list_size, const void* saved,
                      const float* dscores, const void* loss_ws, void* bwd_ws, float* grads, void* stream);

/* Same, with the NA / IPW loss (ultr_softmax_ce) FUSED into the backward kernel's prologue: takes the scores
 * and the feed's labels instead of dscores.  dscores_out may be NULL.  Identical results to
 * ultr_softmax_ce + ultr_dnn_backward (tests/test_gpu_parity.py::test_fused_softmax_backward). */
int ultr_dnn_backward_softmax(const ultr_dnn_desc* d, const float* params, const float* features, int64_t n_docs,
                              const int32_t* docids, int32_t batch, int32_t list_size, const void* saved,
                              const float* scores, const float* labels, const float* pw, const float* ipw_table,
                              int32_t n_ipw, float* dscores_out, void* loss_ws, void* bwd_ws, float* grads, void* stream);

/* partial sums of squares of grads[0..P) -> head of bwd_ws; only needed after an all-reduce */
int ultr_grad_sumsq(float* grads, int64_t n_params, int32_t list_size, void* bwd_ws, void* stream);

/* ---- a4 / a7 / a8: listwise softmax cross entropy (NA, IPW) -------------------------
 * Replaces BaseAlgorithm.softmax_loss + softmax_cross_entropy_with_logits
 * (base_algorithm.py:18-30, 309-330) and, when ipw_table != NULL, the per-list Python loop
 * over BasicPropensityEstimator.getPropensityForOneList (ipw_rank.py:115-128,
 * propensity_estimator.py:22-42):  pw[b,l] = labels[l,b] > 0 ? ipw_table[min(l,n_ipw-1)] : 0.
 * pw (explicit [B, L] weights) and ipw_table may both be NULL (NA: weights = 1).
 * Writes dscores[b,l] = softmax(s_b)_l * S_b - w_bl   (the gradient times the global
 * normaliser D = sum w) and per-workgroup partial sums of (loss_sum, D) into loss_ws.
 * list_size up to 4095 (64 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_softmax_ce(const float* scores, const float* labels, const float* pw, const float* ipw_table,
                    int32_t n_ipw, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- a9: DLA dual loss ---------------------------------------------------------------
 * Replaces DLA.train's loss section (dla.py:196-237) + DenoisingNet.forward (dla.py:33-48)
 * + get_normalized_weights (dla.py:287-306).  prop_params = [W(L) | bias] of the
 * DenoisingNet's Linear(L,1).  logits_to_prob: 0 softmax, 1 sigmoid (dla.py:21-22).
 * dscores = rank-loss gradient x D_rank (the ranker_loss_weight is applied by the update);
 * loss_ws gets (rank_loss_sum, D_rank, exam_loss_sum, D_exam) and the per-position sums of
 * d(exam_loss)/d(propensity) x D_exam.
 * list_size up to 3276 (64 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_dla_loss(const float* scores, const float* labels, const float* prop_params, int32_t logits_to_prob,
                  int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- a10: PairDebias pairwise loss ---------------------------------------------------
 * Replaces the 2-level Python pair loop of PairDebias.train (pairwise_debias.py:142-157)
 * + pairwise_cross_entropy_loss (base_algorithm.py:228-248), including the reference's xB
 * broadcast inflation; `batch_total` is the GLOBAL batch size (== batch on one GPU).
 * loss_ws gets loss_sum and the per-position t_plus_loss / t_minus_loss sums.
 * list_size up to 585 (160 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_pairdebias_loss(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                         int32_t batch, int32_t list_size, int32_t batch_total, float* dscores, void* loss_ws,
                         void* stream);

/* ---- a11: LambdaRank -----------------------------------------------------------------
 * Replaces LambdaRank.train's loss section (lambda_rank.py:116-135) + dcg/compute_delta_ndcg
 * (lambda_rank.py:247-291): per-list descending sort, pairwise delta-NDCG-weighted
 * BCE-with-logits on sigma(s_i - s_j), batch-global natural-log IDCG (kept separate as D).
 * list_size up to 531 (160 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_lambdarank_loss(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                         float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws,
                         void* stream);

/* ---- next row 8f.3: RegressionEM -----------------------------------------------------
 * Replaces RegressionEM.train's estimation + loss section (regression_EM.py:128-151, get_bernoulli_sample
 * :20-34): gamma = sigmoid(s); posteriors with the propensity [L]; pseudo-labels ceil(p_r1 - u) with u from
 * `uniforms` [B, L] (teacher-forced) or, when NULL, Philox keyed by (seed, step); BCE-with-logits, mean over
 * B*L (the count is left in the tail as D).  loss_ws also gets the per-position sums of the M-step
 * (regression_EM.py:180-183), applied by ultr_apply_update (aux = propensity).  pseudo_labels_out may be NULL.
 * list_size up to 8190 (64 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_regem_loss(const float* scores, const float* labels, const float* propensity, const float* uniforms,
                    uint64_t seed, uint64_t step, int32_t batch, int32_t list_size, float* dscores,
                    float* pseudo_labels_out, void* loss_ws, void* stream);

/* ---- TwoTower: joint click likelihood of a relevance and an observation tower (additive within ABI 8) ----
 * The project's own pointwise learner (PAL's "shallow tower"); the click model of RegressionEM fitted by gradient steps.
 * scores [B, L] = the relevance tower s; bias_logits [L] = the observation tower theta (one logit per position); click
 * c = min(labels[l, b], 1) (graded labels clamp, fractional ones in [0, 1] are taken as they are).
 * combination 0 (product): p = sigmoid(s) sigmoid(theta_l); ULTR_TWOTOWER_SUM: p = sigmoid(s + theta_l).
 * Element loss -c log p - (1 - c) log(1 - p), summed over the positions of a list; D = the number of lists (the update divides).
 * Evaluated without cancellation: log sigmoid(x) = min(x, 0) - log1p(exp(-|x|)); product: q = 1 - p = sigmoid(-s) +
 * sigmoid(s) sigmoid(-theta), log(1 - p) = log1p(-p) where p < 0.5 and log q otherwise, r = (1 - c) p / q - c,
 * dl/ds = sigmoid(-s) r, dl/dtheta = sigmoid(-theta) r; sum: BCE-with-logits of z = s + theta, dl/ds = dl/dtheta = sigmoid(z) - c.
 * docids [L, B] != NULL: a PAD position (id < 0 or >= n_docs) adds nothing to the loss, gets dscores exactly 0 and adds nothing to
 * theta's gradient; docids == NULL: every position counts (a PAD as an unclicked document, RegressionEM's convention).
 * Writes dscores = dl/ds (x D) and the step tail [sum l, lists, 0, 0, sum_b dl/dtheta_l at 4 + l ...]; no atomics, the same inputs
 * give the same bits.  ultr_apply_update (ULTR_ALGO_TWOTOWER, aux = theta) clips the two towers separately and steps theta with the
 * descriptor's optimizer at propensity_learning_rate.
 * list_size up to 8190 (64 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched.
 * ULTR_E_BADARG: a missing pointer, batch <= 0, list_size <= 0, a combination other than 0 / ULTR_TWOTOWER_SUM, docids with n_docs < 0. */
#define ULTR_TWOTOWER_SUM 1  /* also bit 0 of ultr_update_desc::logits_to_prob */
#define ULTR_TWOTOWER_MASK 2 /* bit 1 of ultr_update_desc::logits_to_prob: ultr_train_step passes its docids to the loss */
int ultr_twotower_loss(const float* scores, const float* labels, const float* bias_logits, int32_t combination, const int32_t* docids,
                       int64_t n_docs, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- PLRank: Plackett-Luce policy gradient of the expected DCG@K (PL-Rank, Oosterhuis 2021; additive within ABI 8) ----
 * The project's own counterfactual learner of a ranking metric; the law is DESIGN.md section 4d.  Per list of L positions:
 *   valid document: docids[l, b] in [0, n_docs); a PAD is never drawn, has rho = 0 and gets dscores exactly 0;
 *   rho_l = w_l gain(labels[l, b]),  w_l = pw[b, l] (pw != NULL), else ipw_table[min(l, n_ipw - 1)] (ipw_table != NULL), else 1;
 *   gain 0 (ULTR_PLRANK_GAIN_LINEAR): y;  ULTR_PLRANK_GAIN_EXP2: 2^y - 1;
 *   policy e_d = exp(s_d - max over valid s); n_samples rankings per list, each the exponential race of the online feeds at
 *   tau = 1 (PADs staged as -inf): descending keys, the documents of fp32 probability 0 and the PADs behind the n_pos drawn ones in
 *   index order; the race uniform of position l in sample n is word l % 4 of Philox(key(rng_seed, rng_step); b, n, l / 4,
 *   0x504C524B);  K = cutoff (0: L),  K_eff = min(K, n_pos);
 *   per sample, ranks from 0:  theta_k = 1 / log2(k + 2);  Z_k = sum of e over the valid documents at ranks >= k;
 *   FR_k = sum_{x = k}^{K_eff - 1} theta_x rho_{y_x};  RI_i = sum_{k <= i} FR_k / Z_k;  DR_i = sum_{k <= i} theta_k / Z_k;
 *   a valid document d at rank r, i = min(r, K_eff - 1):  g_d = [r < K_eff] FR_{r + 1} + e_d (rho_d DR_i - RI_i);
 *   dscores[b, d] = -(1 / N) sum_n g_d;  step tail [-(1 / N) sum_n FR_0, 1, 0, 0, zeros]: D counts lists (the update divides).
 * The estimator is unbiased for d E[sum_{k < K} theta_k rho_{y_k}] / d s.  No atomics: the same inputs, seed and step give the same
 * bits.  perm_out: NULL or [B, n_samples, L] int32, the order every sample was drawn in.
 * list_size up to 465 (160 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched.
 * ULTR_E_BADARG: a missing scores / labels / docids / dscores / loss_ws, batch <= 0, list_size <= 0, n_docs < 0, cutoff < 0,
 * n_samples outside 1 .. 4095, a gain other than the two, ipw_table with n_ipw <= 0.
 * Out of scope: data parallelism, an NDCG-normalised reward, sampling at tau != 1. */
#define ULTR_PLRANK_GAIN_LINEAR 0
#define ULTR_PLRANK_GAIN_EXP2 1
#define ULTR_PLRANK_MAX_SAMPLES 4095
/* ultr_update_desc::logits_to_prob of a ULTR_ALGO_PLRANK step: bits 0-11 min(cutoff, 4095), bits 12-23 n_samples, bit 24 the exp2 gain */
#define ULTR_PLRANK_PACK(cutoff, n_samples, gain) \
  ((int32_t)(((cutoff) > 4095 ? 4095 : (cutoff)) | ((n_samples) << 12) | (((gain) & 1) << 24)))
int ultr_plrank_loss(const float* scores, const float* labels, const float* pw, const float* ipw_table, int32_t n_ipw,
                     const int32_t* docids, int64_t n_docs, int32_t cutoff, int32_t n_samples, int32_t gain, uint64_t rng_seed,
                     uint64_t rng_step, int32_t batch, int32_t list_size, float* dscores, int32_t* perm_out, void* loss_ws, void* stream);

/* ---- AffineRank: listwise softmax loss under the affine correction of trust bias (additive within ABI 8) ----
 * The project's own counterfactual learner for clicks that follow P(click | rank k, relevance gamma) = alpha_k gamma + beta_k; the law
 * is DESIGN.md section 4e.  Per list of L positions, c = labels[l, b] as it is, k = min(l, n_aff - 1):
 *   live position: docids == NULL, or docids[l, b] in [0, n_docs);
 *   w_l = live ? (c - beta[k]) / alpha[k] : 0  (the division correctly rounded);  the softmax runs over all L positions (a PAD stays in
 *   the denominator, as in ultr_softmax_ce);  loss_b = sum_l w_l (lse - s_l);
 *   dscores[b, l] = softmax_l W_b - w_l,  W_b = sum_l w_l accumulated in double and rounded once.
 * w_l, W_b and loss_b may be negative or zero.  Step tail [sum_b loss_b, 1 per list, 0, 0, zeros]: D counts lists (the update divides).
 * No atomics: the same inputs give the same bits.  alpha [n_aff] must be > 0 (the caller's check; learning_algorithm.AffineRank makes it).
 * list_size up to 4095 (64 KiB of LDS, ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched.
 * ULTR_E_BADARG: a missing scores / labels / alpha / beta / dscores / loss_ws, batch <= 0, list_size <= 0, n_aff <= 0, docids with
 * n_docs < 0.
 * In ultr_train_step: ipw_table = [alpha(n) | beta(n)], n_ipw = n, ultr_update_desc::logits_to_prob bit 0 = PADs are masked
 * (ULTR_AFFINE_MASK).  Out of scope: estimating (alpha, beta) from clicks, data parallelism. */
#define ULTR_AFFINE_MASK 1
int ultr_affine_loss(const float* scores, const float* labels, const float* alpha, const float* beta, int32_t n_aff,
                     const int32_t* docids, int64_t n_docs, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- PRSrank: propensity-ratio-scored LambdaRank -------------------------------------
 * Replaces PRSrank.train's propensity + loss section (prs_rank.py:94-176) + dcg/compute_delta_ndcg
 * (prs_rank.py:207-251): ipw[l] = ipw_table[min(l, n_ipw-1)] for EVERY position (clicked or not), pw = 1/ipw
 * (0 where ipw == 0), per-list descending sort, prs_ij = ipw_i * pw_j on the pairs i < j of the sorted order,
 * delta-NDCG-weighted F.binary_cross_entropy (logs clamped at -100) of 1 / (exp(-sigma (s_i - s_j)) + 1),
 * batch-global natural-log IDCG (kept separate as D).  The gradient is autograd's through that composition,
 * including its explosion where x rounds to 1 and its NaN where exp overflows in the lower triangle.
 * list_size up to 952 (160 KiB of LDS, ultr_loss_lds_bytes), for ultr_prs_loss_pw too; beyond, ULTR_E_UNSUPPORTED and nothing is
 * launched. */
int ultr_prs_loss(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, float sigma,
                  int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);
/* The same with a weight per list entry (additive within ABI 8): ipw_bl [B, L], indexed by PRESENTATION position, replaces
 * ipw_table[min(l, n_ipw-1)] - the weights of an estimator that looks at the list's clicks (ultr_history_pw, all_positions = 1).
 * Everything else, pw = 1/ipw (0 where ipw == 0) included, is ultr_prs_loss.  ultr_train_step with ULTR_ALGO_PRS takes this path
 * when ultr_step_args::pw is set.  ULTR_E_BADARG: a missing pointer, batch <= 0, list_size <= 0. */
int ultr_prs_loss_pw(const float* scores, const float* labels, const float* ipw_bl, float sigma, int32_t batch, int32_t list_size,
                     float* dscores, void* loss_ws, void* stream);

/* ---- PDGD: Pairwise Differentiable Gradient Descent (online) ---------------------------
 * Replaces PDGD.train's pair construction and loss (pdgd.py:107-205) over the list_size positions the forward scored
 * (max_candidate_num there): e = exp(tau (s - max s)) in fp32, zeroed for PADs (docids[l,b] == n_docs) at l < cutoff
 * only (pdgd.py:120-126); pairs (l, k) with l < cutoff valid and label_l > 0, k in 0 .. l+1, k < cutoff, k valid and
 * label_k < label_l (pdgd.py:138-172); weight 1 / (1 + exp(min(delta, 20))) with delta the flipped list's sum of log
 * suffix sums minus the original's (pdgd.py:128-134, 160-176), a constant; loss = sum of -w e^{s_l} / (e^{s_l} + e^{s_k}) on
 * the raw scores (pdgd.py:193-205), its gradient autograd's through that expression (NaN where exp overflows).
 * Plain sum (D = 1).  Deterministic (no atomics).  list_size up to 256 (one thread per position; 136 KiB of LDS there,
 * ultr_loss_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_pdgd_loss(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, float tau,
                   int32_t cutoff, int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- long lists: PairDebias, LambdaRank, PRSrank beyond 585 / 531 / 952 documents (additive within ABI 8) ----
 * The same losses from kernels that split the OWNED positions over the workgroup's 16 waves (each lane walks every partner, its
 * sums stay in registers), so their LDS is O(list_size).  Arguments, outputs, the step tail and the ULTR_E_BADARG rules are those
 * of the short entries above; a position's sums are one ascending fp32 chain over the partners, so the results agree with the
 * short kernels' to rounding, not bit for bit.  Every list_size from 1 up to the bound is accepted.  One workgroup and one tail
 * partial per list (ultr_loss_part_count, ultr_loss_workspace_bytes as before); no atomics, the same inputs give the same bits.
 * ultr_train_step takes these for a list the short kernel refuses, and only for such a list (decided before anything is launched).
 *
 * Dynamic LDS in bytes of the long kernel of `algo` at list_size, read from the layout the kernel carves its LDS with (host-only).
 * ULTR_E_UNSUPPORTED beyond 160 KiB; ULTR_E_BADARG: list_size <= 0, an algorithm other than ULTR_ALGO_PAIRDEBIAS,
 * ULTR_ALGO_LAMBDARANK, ULTR_ALGO_PRS. */
int64_t ultr_loss_long_lds_bytes(int32_t algo, int32_t list_size);
/* the longest list the long kernel of `algo` accepts (6823 / 3149 / 3721); ULTR_E_BADARG for an algorithm without one */
int32_t ultr_loss_long_max_list(int32_t algo);
/* ultr_pairdebias_loss for long lists.
 * list_size up to 6823 (160 KiB of LDS, ultr_loss_long_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_pairdebias_loss_long(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                              int32_t batch, int32_t list_size, int32_t batch_total, float* dscores, void* loss_ws,
                              void* stream);
/* ultr_lambdarank_loss for long lists.
 * list_size up to 3149 (160 KiB of LDS, ultr_loss_long_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_lambdarank_loss_long(const float* scores, const float* labels, const float* t_plus, const float* t_minus,
                              float sigma, int32_t batch, int32_t list_size, float* dscores, void* loss_ws,
                              void* stream);
/* ultr_prs_loss for long lists.
 * list_size up to 3721 (160 KiB of LDS, ultr_loss_long_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_prs_loss_long(const float* scores, const float* labels, const float* ipw_table, int32_t n_ipw, float sigma,
                       int32_t batch, int32_t list_size, float* dscores, void* loss_ws, void* stream);
/* ultr_prs_loss_pw for long lists.
 * list_size up to 3721 (160 KiB of LDS, ultr_loss_long_lds_bytes); beyond, ULTR_E_UNSUPPORTED and nothing is launched. */
int ultr_prs_loss_pw_long(const float* scores, const float* labels, const float* ipw_bl, float sigma, int32_t batch,
                          int32_t list_size, float* dscores, void* loss_ws, void* stream);

/* ---- next row 8f.1: the SetRank ranking model --------------------------------------------
 * Replaces SetRank.build / Encoder.forward (ranking_model/SetRank.py:143-156, 229-255) and its autograd
 * backward: input LayerNorm (eps 1e-6) -> FFN(F -> dff -> d_model) -> num_layers x [multi-head self-attention
 * WITHOUT projections (heads = slices of x) -> dense -> residual + LayerNorm -> FFN -> residual + LayerNorm]
 * -> FFN(d_model -> dff -> 1).  fp32 (attention optionally with fp16 operands, see attention_dtype); every kernel is
 * hand-written: the Linear layers run on the library's LDS-tiled matrix-core GEMM with fused bias / ReLU epilogues.
 * params: flat vector in SetRank.state_dict() order (Encoder_layer.input_layer_norm, input_embedding.{0,2},
 * output_layer.{0,2}, then per encoder: mha.dense, ffn.{0,2}, layernorm1, layernorm2).
 * forward: scores [B, L]; `saved` (ultr_setrank_saved_bytes) receives every activation the backward needs (it doubles as
 * scratch); a forward that no backward follows - validation - takes ultr_setrank_score and its smaller buffer.
 * Any list_size: up to 256 documents the one-pass attention kernels run,
 * beyond them (ULTR_SR_ATTN_LONG_MIN, default 257, lowers the hand-over) the keys stream through LDS in tiles with a running row
 * maximum and sum (fp32 matrix cores at head depth 16 / 32 / 64, a scalar kernel at every other up to 420: its rows sit in LDS,
 * as the one-pass scalar kernel's do - beyond, ULTR_E_UNSUPPORTED before anything is launched); what bounds the forward is
 * batch * list_size <= 0x7fffffff / 4 and the size of `saved`.
 * backward: dscores [B, L] from any ultr_*_loss kernel (x D convention), loss_ws/n_loss_parts = that kernel's
 * partials; writes grads [P + step tail]; follow with ultr_grad_sumsq + ultr_apply_update(wt = NULL).
 * list_size <= 128 on the matrix-core attention path (head depth 16 / 32 / 64), <= 120 otherwise - a forward at a longer list is an
 * evaluation (ULTR_E_UNSUPPORTED from the backward) - unless the descriptor carries ULTR_MODEL_SR_STREAM_BWD: then any list_size,
 * through the streaming attention backward (fp32 matrix cores at head depth 16 / 32 / 64, a scalar kernel at every other up to 228;
 * deterministic, no atomics).
 * `saved`, `workspace` (and `work` of ultr_setrank_score) are to be 16-byte aligned - what a torch allocation gives; the features
 * pointer needs its natural 4-byte alignment only (a caller may pass a slice of a larger matrix: the fused embedding launch steps
 * aside for the separate launches where it is not 16-byte aligned). */
enum ultr_attention_dtype { ULTR_ATTN_FP32 = 0, ULTR_ATTN_FP16 = 1 };
typedef struct ultr_setrank_desc {
  int32_t feature_size, d_model, num_heads, num_layers, dff;
  /* operand type of the self-attention products (ABI 2).  ULTR_ATTN_FP32 (default): exact fp32 matrix cores, the 1e-5
   * parity path.  ULTR_ATTN_FP16: fp16 operands with fp32 accumulation on v_mfma_f32_16x16x32_f16 (what BASELINE
   * config 5 names); scores / softmax / gradients algebra stay fp32; parity is ORDERING-level (~1e-3 relative), so it is
   * opt-in.  Needs head depth 32 or 64 and list_size <= 128, otherwise the fp32 kernels run (the streaming kernels of the long
   * lists are fp32 only: ULTR_ATTN_FP16 at list_size 300 runs them). */
  int32_t attention_dtype;
  int32_t flags;  /* ABI 6: ULTR_MODEL_FP32_PRODUCTS - the Linear products and d x d weight gradients of this model on the fp32 matrix cores;
                   * ULTR_MODEL_SR_STREAM_BWD - streaming attention backward beyond the one-pass bounds (see the define) */
} ultr_setrank_desc;
int64_t ultr_setrank_param_count(const ultr_setrank_desc* c);
int64_t ultr_setrank_saved_bytes(const ultr_setrank_desc* c, int64_t n_rows);
int64_t ultr_setrank_workspace_bytes(const ultr_setrank_desc* c, int64_t n_rows);
/* ABI 6: float offset into `saved` of the word ultr_setrank_forward raises ULTR_H3_FLAG_* bits in when it builds the split-half
 * planes of the weights (zeroed by every forward; ultr_update_desc::range_flag); -1 on a bad desc */
int64_t ultr_setrank_range_flag_offset(const ultr_setrank_desc* c, int64_t n_rows);
int ultr_setrank_forward(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                         const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* saved, void* stream);
int ultr_setrank_backward(const ultr_setrank_desc* c, const float* params, int32_t batch, int32_t list_size, const void* saved,
                          const float* dscores, const void* loss_ws, int32_t n_loss_parts, void* workspace, float* grads,
                          void* stream);
/* Which attention kernel family a shape takes (additive within ABI 8; host-only, launches nothing): the value of THE dispatch the
 * forward (backward = 0) / the backward (backward = 1; the split-half knobs as for layer 0) goes through at list_size, under the knobs
 * as last read (ultr_config_reload), or ULTR_E_UNSUPPORTED where the call itself would refuse; ULTR_E_BADARG on a bad desc. */
enum ultr_setrank_attn_path_id {
  ULTR_SR_ATTN_SCALAR = 0,       /* one wave per query row, the head slice in LDS */
  ULTR_SR_ATTN_MFMA = 1,         /* fp32 matrix cores, the score row in registers (list_size <= 128) */
  ULTR_SR_ATTN_F16 = 2,          /* fp16 operands (ULTR_ATTN_FP16) */
  ULTR_SR_ATTN_SPLIT_HALF = 3,   /* hi / lo fp16 operands (backward only) */
  ULTR_SR_ATTN_LONG_MFMA = 4,    /* keys / partner tokens streamed in tiles, fp32 matrix cores */
  ULTR_SR_ATTN_LONG_SCALAR = 5   /* keys / partner tokens streamed in tiles, scalar */
};
int32_t ultr_setrank_attn_path(const ultr_setrank_desc* c, int32_t list_size, int32_t backward);
/* Which launches a step takes (additive within ABI 8; host-only, launches nothing): the route ultr_setrank_forward and
 * ultr_setrank_backward decide once per call at batch x list_size - dropout != 0: of a dropout step - under the knobs as last read
 * (ultr_config_reload) and the descriptor's flags, for 16-byte aligned `saved` / `workspace` and a feature matrix the fused embedding
 * launch takes (16-byte aligned, below 2 GiB: the forward tests that at the launch), with the CU count the forward itself reads (256
 * where no device answers).  ULTR_E_BADARG: a bad desc, a NULL out, batch <= 0 or list_size <= 0. */
typedef struct ultr_setrank_route_info {
  int32_t embed;          /* 1: gather + input LayerNorm + embedding FFN as one launch */
  int32_t block;          /* behind the attention of every encoder block: 0 separate launches, 1 the round-5 kernel, 2 the persistent kernel */
  int32_t head_rides;     /* the output FFN runs inside the last block's launch */
  int32_t skip_out1;      /* out1 is neither written by the forward nor read by the backward */
  int32_t bwd_head, bwd_blocks, bwd_embed; /* the fused backward launches (ULTR_SR_BWD_FUSED bits 2, 1, 4) */
  int32_t rows_per_tile, tiles, workgroups; /* the persistent launches, both directions (0: none run) */
  int32_t block_rows, embed_rows; /* rows per workgroup of the round-5 block / embedding kernel (0: it does not apply) */
  int32_t wgrad_split;    /* chunks of whole lists of the plain weight-gradient kernel */
  int32_t reserved[3];    /* 0 */
} ultr_setrank_route_info;
int ultr_setrank_route(const ultr_setrank_desc* c, int32_t batch, int32_t list_size, int32_t dropout, ultr_setrank_route_info* out);
/* The evaluation forward (additive within ABI 8): the scores of ultr_setrank_forward, bit for bit on every route and attention family,
 * and no record for a backward.  `work` (ultr_setrank_score_bytes; about F + dff + 4 d_model floats per row whatever num_layers, plus
 * the split-half planes) holds only what one launch hands to the next: x_l / x_{l+1} alternate between two buffers, the attention's
 * output has one, the separate launches share one buffer per row width; statistics rows, lse and - on the fused launches - every
 * row the backward alone reads are not stored.  The planes are rebuilt per call and the range word raised as in the training
 * forward, at float offset ultr_setrank_score_range_flag_offset of `work` (-1 on a bad desc).  No dropout.
 * work_bytes < ultr_setrank_score_bytes(c, batch * list_size): ULTR_E_WORKSPACE, nothing launched; every other refusal is
 * ultr_setrank_forward's. */
int64_t ultr_setrank_score_bytes(const ultr_setrank_desc* c, int64_t n_rows);
int64_t ultr_setrank_score_range_flag_offset(const ultr_setrank_desc* c, int64_t n_rows);
int ultr_setrank_score(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                       const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* work, int64_t work_bytes,
                       void* stream);

/* SetRank's dropout.  Replaces the nn.Dropout(rate) calls of EncoderLayer.forward and Encoder.forward (ranking_model/SetRank.py:103-117,
 * 141-153) at 1 + 2 num_layers sites: 0 behind input_embedding, 1 + 2 l behind encoder l's mha.dense, 2 + 2 l behind its ffn - each on
 * the Linear's output with its bias, before the residual is added; the output FFN has none.
 * keep(site, t, c) is a pure function: word c & 3 of Philox-4x32-10 under the (seed, step) key of the online feeds, counter
 * (t, (stream << 8) | site, c >> 2, 0x5352444F), t = l * batch + b the position-major token, c the column; keep iff
 * u01(word) >= rate in float32; y = keep ? v / (1 - rate) : 0.  Nothing is stored: the backward draws the mask again, so it takes the
 * (seed, step, stream) of its forward.  stream: 0 on one GPU, the rank under data parallelism (< 2^24).
 * A dropout step runs the separate launches in both directions (none of the fused persistent kernels).  dropout == NULL or
 * rate == 0: exactly ultr_setrank_forward / ultr_setrank_backward, bit for bit.  rate outside [0, 1) (or NaN): ULTR_E_BADARG.
 * backward: scratch = ultr_setrank_dropout_workspace_bytes(desc, n_rows) bytes, 16-byte aligned, next to `workspace` (which keeps its
 * size); a missing, unaligned or short scratch: ULTR_E_WORKSPACE.  The forward reads rate, seed, step and stream only. */
typedef struct ultr_setrank_dropout {
  float rate;
  uint64_t seed, step;
  uint32_t stream;
  void* scratch;
  int64_t scratch_bytes;
} ultr_setrank_dropout;
int64_t ultr_setrank_dropout_workspace_bytes(const ultr_setrank_desc* c, int64_t n_rows);
int ultr_setrank_forward_dropout(const ultr_setrank_desc* c, const float* params, const float* features, int64_t n_docs,
                                 const int32_t* docids, int32_t batch, int32_t list_size, float* scores, void* saved,
                                 const ultr_setrank_dropout* dropout, void* stream);
int ultr_setrank_backward_dropout(const ultr_setrank_desc* c, const float* params, int32_t batch, int32_t list_size, const void* saved,
                                  const float* dscores, const void* loss_ws, int32_t n_loss_parts, void* workspace, float* grads,
                                  const ultr_setrank_dropout* dropout, void* stream);

/* ---- the DLCM ranking model (additive within ABI 8) --------------------------------------------
 * Deep Listwise Context Model (Ai, Bi, Guo, Croft, SIGIR 2018); the reference names it (ultra.ranking_model.DLCM) and ships no code.
 * Per list: xh_l = LayerNorm_F(x_l) (eps 1e-5, PAD = the zero row -> beta); a one-layer GRU (torch.nn.GRU's law and layout, gates
 * r, z, n) reads the list from the LAST position to the FIRST from h = 0, o_l = the state after position l, s = o_0;
 * M = tanh(W_phi s + b_phi) as [num_heads, H], m = sum_j v_j M_j, score_l = o_l . m.
 * params: one flat vector, offsets by ultr_dlcm_param_offsets: layer_norm.weight / .bias [F], gru.weight_ih_l0 [3H, F],
 * gru.weight_hh_l0 [3H, H], gru.bias_ih_l0 / .bias_hh_l0 [3H], att_linear.weight [num_heads H, H], att_linear.bias [num_heads H],
 * att_v.weight [1, num_heads].
 * feature_size and hidden_size are multiples of 4 (16-byte rows); every other model is ULTR_E_UNSUPPORTED from the size queries and
 * from the calls, before anything is launched or written.  list_size >= 1 with no bound of the model's own; the recurrent kernels keep
 * 16 lists in LDS: hidden_size <= 848 trains (above 624 the carried state gradient sits in `workspace`), the forward runs up to 1264.
 * forward: docids [L, B] position-major (PAD = n_docs), scores [B, L].  saved != NULL (ultr_dlcm_saved_bytes): the training form, `work`
 * is not read; saved == NULL: the scoring form, the same launches with the same bits writing only what one launch hands to the next
 * into `work` (ultr_dlcm_score_bytes).
 * backward: dscores [B, L] from any ultr_*_loss kernel (x D convention); loss_ws / n_loss_parts: that kernel's partials, folded into
 * the step tail grads [P ..) (NULL / 0: the tail is left alone); workspace: ultr_dlcm_workspace_bytes.  Writes all P gradients; follow
 * with ultr_grad_sumsq + ultr_apply_update(d = NULL, wt = NULL).  No atomics: the same inputs give the same bits.
 * Every buffer is to be 16-byte aligned (ULTR_E_BADARG otherwise). */
typedef struct ultr_dlcm_desc {
  int32_t feature_size, hidden_size, num_heads;
} ultr_dlcm_desc;
/* offsets[0 .. 9) of the nine parameter tensors in the order above, offsets[9] = P; ULTR_E_BADARG on a bad desc */
int ultr_dlcm_param_offsets(const ultr_dlcm_desc* c, int64_t* offsets);
/* bytes for any batch x list_size = n_rows; ULTR_E_BADARG / ULTR_E_UNSUPPORTED as the calls */
int64_t ultr_dlcm_saved_bytes(const ultr_dlcm_desc* c, int64_t n_rows);
int64_t ultr_dlcm_score_bytes(const ultr_dlcm_desc* c, int64_t n_rows);
int64_t ultr_dlcm_workspace_bytes(const ultr_dlcm_desc* c, int32_t batch, int32_t list_size);
int ultr_dlcm_forward(const ultr_dlcm_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                      int32_t batch, int32_t list_size, float* scores, void* saved, void* work, void* stream);
int ultr_dlcm_backward(const ultr_dlcm_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                       int32_t batch, int32_t list_size, const void* saved, const float* dscores, const void* loss_ws,
                       int32_t n_loss_parts, void* workspace, float* grads, void* stream);

/* ---- the GSF ranking model (additive within ABI 8) ---------------------------------------------
 * Groupwise Scoring Function (Ai, Wang, Bendersky et al., ICTIR 2019); the reference's README lists it and ships no code.
 * Per list of L presented positions (m = group_size): perm[p] = the presented position at place p (NULL: the identity); group g
 * (one per place) holds in slot j the document at place (g + j) mod L, a PAD (document id n_docs) as the zero row;
 * u_g = LayerNorm_{mF}(the m rows side by side), eps 1e-5; then the DNN's layers on it, [Linear -> act -> LayerNorm] x n_hidden and
 * a Linear of m outputs o_g; score[perm[p]] = sum_j o_{(p - j) mod L}[j], summed in the order j = 0 .. m - 1.
 * params: one flat vector in the DNN's order, offsets by ultr_gsf_param_offsets: per Linear layer LayerNorm weight / bias [K_j], weight
 * [M_j, K_j], bias [M_j] with K_0 = m F and M_last = m; at m = 1 the layout and the model are ultr_dnn_desc's.
 * feature_size and every hidden width are multiples of 4 (16-byte rows), 1 <= group_size <= 8; every other model is
 * ULTR_E_UNSUPPORTED (not a model at all: ULTR_E_BADARG) from the size queries and from the calls, before anything is launched or
 * written.  Any batch >= 1, list_size >= 1 (m > L: a document recurs in a group).
 * shuffle: perm [B, L], list b by Fisher-Yates from the identity, i = L - 1 .. 1: r = philox_word(philox_step_key(seed, step), b, 0,
 * i, ULTR_GSF_SHUFFLE_TAG), j = (r (i + 1)) >> 32, swap entries i and j.  A pure function of (seed, step, list).
 * forward: docids [L, B] position-major (PAD = n_docs), scores [B, L].  saved != NULL (ultr_gsf_saved_bytes): the training form, `work`
 * is not read; saved == NULL: the scoring form, the same launches with the same bits on `work` (ultr_gsf_score_bytes).  perm must be
 * a permutation per list; an entry outside 0 .. L - 1 reads as a PAD and writes no score.
 * backward: dscores [B, L] from any ultr_*_loss kernel (x D convention), d o_g[j] = dscores[perm[(g + j) mod L]]; perm as the forward's;
 * loss_ws / n_loss_parts: that kernel's partials, folded into the step tail grads [P ..) (NULL / 0: the tail is left alone);
 * workspace: ultr_gsf_workspace_bytes.  Writes all P gradients; follow with ultr_grad_sumsq + ultr_apply_update(d = NULL, wt = NULL).
 * No atomics: the same inputs give the same bits.  Every buffer is to be 16-byte aligned (ULTR_E_BADARG otherwise). */
typedef struct ultr_gsf_desc {
  int32_t feature_size, group_size, n_hidden;
  int32_t hidden[ULTR_MAX_HIDDEN];
  int32_t activation; /* as ultr_dnn_desc: 0 elu, 1 relu, 2 tanh, 3 sigmoid */
} ultr_gsf_desc;
/* P, or 0 on a bad desc */
int64_t ultr_gsf_param_count(const ultr_gsf_desc* c);
/* offsets[4 j .. 4 j + 4) = LayerNorm weight, LayerNorm bias, Linear weight, Linear bias of layer j <= n_hidden; ULTR_E_BADARG on a bad desc */
int ultr_gsf_param_offsets(const ultr_gsf_desc* c, int64_t* offsets);
/* bytes for any batch x list_size = n_rows; ULTR_E_BADARG / ULTR_E_UNSUPPORTED as the calls */
int64_t ultr_gsf_saved_bytes(const ultr_gsf_desc* c, int64_t n_rows);
int64_t ultr_gsf_score_bytes(const ultr_gsf_desc* c, int64_t n_rows);
int64_t ultr_gsf_workspace_bytes(const ultr_gsf_desc* c, int32_t batch, int32_t list_size);
int ultr_gsf_shuffle(uint64_t seed, uint64_t step, int32_t batch, int32_t list_size, int32_t* perm, void* stream);
int ultr_gsf_forward(const ultr_gsf_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                     const int32_t* perm, int32_t batch, int32_t list_size, float* scores, void* saved, void* work, void* stream);
int ultr_gsf_backward(const ultr_gsf_desc* c, const float* params, const float* features, int64_t n_docs, const int32_t* docids,
                      const int32_t* perm, int32_t batch, int32_t list_size, const void* saved, const float* dscores, const void* loss_ws,
                      int32_t n_loss_parts, void* workspace, float* grads, void* stream);

/* ---- a5 (clip) + a6 (optimizer) + EM / propensity updates ----------------------------
 * Replaces torch.nn.utils.clip_grad_norm_ + Adagrad.step / SGD.step
 * (base_algorithm.py:223-226; ipw_rank.py:96), DLA.separate_gradient_update
 * (dla.py:141-177: per-model clip, fresh = stateless Adagrad), and the t_plus/t_minus EM
 * updates (pairwise_debias.py:159-163, lambda_rank.py:136-142). */
enum ultr_algo { ULTR_ALGO_SOFTMAX = 0, ULTR_ALGO_DLA = 1, ULTR_ALGO_PAIRDEBIAS = 2, ULTR_ALGO_LAMBDARANK = 3, ULTR_ALGO_REGEM = 4,
                 ULTR_ALGO_PRS = 5, ULTR_ALGO_PDGD = 6,
                 /* DBGD / MGD: grads from ultr_dbgd_grad_args, loss in the step tail, D = 1 (no l2_loss) */
                 ULTR_ALGO_DBGD = 7,
                 /* TwoTower (additive within ABI 8): ultr_twotower_loss, aux = the observation tower's logits [L].  The value 8 is
                  * left out and stays ULTR_E_BADARG everywhere: tests/test_adam_cpu.py holds `algo = 8` to be a bad descriptor. */
                 ULTR_ALGO_TWOTOWER = 9,
                 /* PLRank (additive within ABI 8): ultr_plrank_loss, no aux; cutoff, sample count and gain in logits_to_prob.  The
                  * value 10 is left out as 8 is and stays ULTR_E_BADARG everywhere: tests/test_twotower_cpu.py holds `algo = 10` to
                  * be a bad descriptor. */
                 ULTR_ALGO_PLRANK = 11,
                 /* AffineRank (additive within ABI 8): ultr_affine_loss, no aux; ipw_table carries [alpha | beta], the PAD-mask flag
                  * rides in logits_to_prob. */
                 ULTR_ALGO_AFFINE = 12 };
/* ULTR_OPT_ADAM: torch.optim.Adam with its defaults (no weight decay, no amsgrad), applied to the gradient Adagrad / SGD get - after
 * the 1 / D scaling, the l2_loss term and the clip.  For step t = 1, 2, ...:
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * The moments persist for every algorithm, DLA included (its Adagrad is stateless only because the reference rebuilds its optimizers
 * every step); DLA's propensity parameters aux[0 .. L] keep moments of their own and step with propensity_learning_rate. */
enum ultr_opt { ULTR_OPT_ADAGRAD = 0, ULTR_OPT_SGD = 1, ULTR_OPT_ADAM = 2 };
#define ULTR_ADAM_BETA1 0.9
#define ULTR_ADAM_BETA2 0.999
#define ULTR_ADAM_EPS 1e-8

typedef struct ultr_update_desc {
  int32_t algo;            /* ultr_algo */
  int32_t optimizer;       /* ultr_opt (grad_strategy 'ada' / 'sgd' / 'adam') */
  int32_t list_size;       /* L */
  int32_t logits_to_prob;  /* DLA: 0 softmax, 1 sigmoid.  TwoTower (same field, the struct's layout is unchanged): bit 0 = the towers
                            * combine as a sum (ULTR_TWOTOWER_SUM), bit 1 = PAD positions are masked (ULTR_TWOTOWER_MASK).  PLRank: ULTR_PLRANK_PACK(cutoff, n_samples, gain).
                            * AffineRank: bit 0 = PAD positions are masked (ULTR_AFFINE_MASK) */
  int64_t n_params;        /* P */
  float learning_rate;
  float max_gradient_norm; /* <= 0 disables clipping */
  float adagrad_eps;       /* 1e-10; ULTR_OPT_ADAM: Adam's eps (ULTR_ADAM_EPS) */
  float ranker_loss_weight;     /* DLA */
  float propensity_learning_rate; /* DLA, TwoTower (the observation tower's rate) */
  float em_step_size;      /* PairDebias / LambdaRank */
  float regulation_p;      /* PairDebias / LambdaRank */
  /* l2_loss hyper-parameter (ipw_rank.py:154-157, navie_algorithm.py:109-114, pairwise_debias.py:166-169,
   * regression_EM.py:166-169, dla.py:146-150): loss += l2_loss * sum_p ||p||^2 / 2 over the ranking model's parameters, i.e.
   * g += l2_loss * p.  As in the reference, l2_loss > 0 DISABLES the gradient clip for every algorithm but DLA (the
   * `params` generator handed to clip_grad_norm_ is already exhausted by the L2 loop); DLA adds the term
   * to rank_loss (so it is scaled by ranker_loss_weight) and clips the full gradient. */
  float l2_loss;
  /* ---- ABI 4: per-step reporting / safety (all optional) ----
   * guard: device word; when it is non-zero at launch the update changes NOTHING (parameters, optimizer state, aux stay as
   *   they are) - ultr_train_step points it at the communicator's status word, so a rank whose gradient exchange timed
   *   out (or that was told so by a peer) never applies a partly reduced gradient.
   * host_scalars: 16 floats of HOST-mapped pinned memory (device-accessible pointer): block 0 writes scalars_out[0..8) to
   *   [0..8), then the guard word to [8] and `seq` to [9] and [10] (as uint32, system-scope stores, seq LAST).  The host reads
   *   the step scalars by spinning on [9] == seq instead of a stream synchronisation + device-to-host copy.  [10] == seq means
   *   "the LOSS of step seq is in [0]": ultr_train_step raises it EARLIER where it can - single GPU, l2_loss = 0: from the
   *   weight-gradient launch, as soon as the loss is final, while that step's reduction and update still run (the reference's
   *   loss.item() then costs no pipeline bubble: the next step queues behind the update on the stream). */
  const uint32_t* guard;
  float* host_scalars;
  uint32_t seq;
  /* (the four bytes that were reserved as pad_) ULTR_OPT_ADAM: the step count t >= 1 of this update, counted by the HOST beside the
   *   state (one count per state vector, whatever workspace or batch shape a step runs in); ignored by Adagrad and SGD */
  uint32_t adam_t;
  /* ABI 6 - range_flag: optional device word of ULTR_H3_FLAG_* bits raised by whatever builds split-half (fp16 hi / lo) weight
   *   planes for the caller's model; block 0 of the update reports them in host_scalars[8] as ULTR_STATUS_H3_NEAR / _RANGE.
   *   ultr_train_step / ultr_apply_update with `wt` find the DNN's own word themselves (NULL is fine); a SetRank caller passes
   *   saved + ultr_setrank_range_flag_offset(). */
  const uint32_t* range_flag;
} ultr_update_desc;

/* floats of `state` for this descriptor (host-only; reads algo, optimizer, list_size, n_params): SGD 0; Adagrad P; Adam 2 P as
 * m[P] | v[P], and for DLA 2 (L + 1) more behind them, m_aux[L + 1] | v_aux[L + 1] (the propensity parameters' moments).
 * TwoTower's observation tower keeps state of its own behind the ranker's: Adagrad P + L (its L accumulators), Adam 2 P + 2 L
 * (m[L] | v[L]).  -1 on a bad descriptor.  A fresh state is all zeros. */
int64_t ultr_opt_state_floats(const ultr_update_desc* u);

/* params/state [P] (ultr_opt_state_floats) updated in place; grads = the buffer ultr_dnn_backward filled (possibly
 * all-reduced).  ULTR_OPT_ADAM: state == NULL or adam_t == 0 is ULTR_E_BADARG (here and in ultr_train_step, before anything is
 * launched), as is an optimizer outside ultr_opt.  aux = prop_params[L+1] (DLA) or [t_plus(L) | t_minus(L)] (PairDebias /
 * LambdaRank), updated in place; NULL for SOFTMAX, PRS, PLRANK and AFFINE.  d + wt (both may be NULL): keep the k-major weight copy
 * in sync with the updated parameters.  bwd_ws = the workspace ultr_dnn_backward (or
 * ultr_grad_sumsq) left the sum-of-squares partials in.
 * scalars_out[16]: [0] loss [1] ranker grad norm (pre-clip) [2] clip coef [3] D
 *                  [4] rank_loss (DLA) [5] exam_loss (DLA) [6] propensity grad norm (DLA; TwoTower: the observation tower's,
 *                  pre-clip) [7] sum g^2
 *                  [8] sum p^2  [9] sum g.p  (written by a pre-pass only when l2_loss > 0)  [10..16) reserved
 * wt: NULL (only params are written), or the copies on a 16-byte boundary; one off it is refused with ULTR_E_BADARG and nothing
 * is launched (the operand contract, ultr_dnn_forward).  params needs 4-byte alignment only. */
int ultr_apply_update(const ultr_update_desc* u, const ultr_dnn_desc* d, float* params, float* wt, float* state,
                      const float* grads, float* aux, const void* bwd_ws, float* scalars_out, void* stream);

/* ---- one call per training step -----------------------------------------------------------
 * ultr_dnn_forward -> ultr_<loss by upd->algo> -> ultr_dnn_backward -> ultr_apply_update, enqueued by ONE host
 * call (what `model.train(input_feed)` does between marshalling the feed and `loss.item()`).  A data-parallel
 * caller sets skip_update, all-reduces `grads`, then calls ultr_grad_sumsq + ultr_apply_update itself.
 * aux: prop_params (DLA) or [t_plus | t_minus] (PairDebias / LambdaRank) or propensity [L] (RegressionEM) or the observation
 * tower's logits [L] (TwoTower) or NULL.
 * ipw_table / n_ipw: the IPW_list of IPW (SOFTMAX) and PRS; pw: explicit [B, L] weights instead (SOFTMAX: ultr_softmax_ce's pw;
 * PRS: ultr_prs_loss_pw's ipw_bl).  sigma: LambdaRank and PRS.
 * PDGD (no IPW table, no sigma): sigma carries tau and n_ipw the cutoff (selection_bias_cutoff); docids / n_docs mark
 * the PADs.
 * wt: the weight copies on a 16-byte boundary, or NULL - every algorithm then runs the separate forward / backward calls on the
 * generic kernels (SOFTMAX included: the fused launch needs the copies) and the update writes params only.  A wt off a 16-byte
 * boundary: ULTR_E_BADARG before anything is launched, skip_update or not (the operand contract, ultr_dnn_forward).  params and
 * features need 4-byte alignment only. */
typedef struct ultr_step_args {
  const ultr_dnn_desc* desc;
  const ultr_update_desc* upd;
  float* params;
  float* wt;
  float* state;
  float* aux;
  const float* features;
  const int32_t* docids;
  const float* labels;
  const float* pw;
  const float* ipw_table;
  float* scores;
  float* dscores;
  void* saved;
  void* loss_ws;
  void* bwd_ws;
  float* grads;
  float* scalars;
  int64_t n_docs;
  int32_t n_ipw;       /* PDGD: the cutoff */
  int32_t batch;
  int32_t list_size;
  int32_t batch_total; /* PairDebias: global batch (0 = batch) */
  int32_t skip_update;
  float sigma;         /* LambdaRank / PRS; PDGD: tau */
  const float* uniforms; /* RegressionEM: [B, L] uniforms of the Bernoulli draw, or NULL = Philox(rng_seed, rng_step) */
  /* (rng_seed / rng_step: also the key of PLRank's sampled rankings; its weights come from pw / ipw_table / n_ipw as SOFTMAX's) */
  uint64_t rng_seed;
  uint64_t rng_step;
  /* data parallel (ABI 3): with a communicator the call runs the WHOLE sharded step - backward, then ultr_comm_allreduce of
   * grads[P + tail] (step number comm_step: the caller counts), then the update - instead of stopping for the host to issue
   * the exchange and the update as two more calls (skip_update = 1 keeps that protocol for a process-group all-reduce). */
  struct ultr_comm* comm;
  uint64_t comm_step;
} ultr_step_args;
int ultr_train_step(const ultr_step_args* a, void* stream);

/* ---- a12 + a13: validation metrics ---------------------------------------------------
 * Replaces remove_padding_for_metric_eval (base_algorithm.py:88-116) and
 * normalized_discounted_cumulative_gain (metrics.py:191-265, 456-495):  pads
 * (docid == n_docs) -> -100000, labels < 0 -> label 0 / score rowmin-1e-6, stable descending
 * sort, gains 2^l - 1, log2 discounts, topn clipped to L, mean over the batch.  As in torch: a NaN
 * score sorts above every number, and a NaN in a list makes its rowmin NaN.
 * ndcg_out[n_topn]; order_out (may be NULL) [B, L] int32 = the descending permutation;
 * masked_out (may be NULL) [B, L] = the masked scores.  ndcg_ws: batch*n_topn floats. */
int ultr_ndcg(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
              int32_t list_size, const int32_t* topn, int32_t n_topn, float* ndcg_out, int32_t* order_out,
              float* masked_out, float* ndcg_ws, void* stream);
/* ABI 7: the same as ONE launch with the result in host-mapped memory.  The wave that finishes last (a device counter the caller
 * provides zeroed once: 4 bytes, reset by every launch) sums the per-list values in ultr_ndcg's order (identical bits), writes
 * ndcg_out and - host_report != NULL: a pinned, device-mapped page of >= 17 floats - host_report[0 .. n_topn) followed by the word
 * host_report[16] = seq.  The host then reads a validation batch's metrics by spinning on that word instead of a stream
 * synchronisation + device-to-host copy (the reference's `.item()` per metric, ipw_rank.py:204-210: 18 us per batch at config 2). */
int ultr_ndcg_report(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                     int32_t list_size, const int32_t* topn, int32_t n_topn, float* ndcg_out, int32_t* order_out,
                     float* masked_out, float* ndcg_ws, uint32_t* counter, float* host_report, uint32_t seq, void* stream);
/* ABI 8: validation() as ONE host call: ultr_dnn_forward (saved = NULL) followed by ultr_ndcg_report of its scores on the same stream
 * (base_algorithm.py:88-154 validation forward + metrics.py:456-495).  Same arguments, same results. */
int ultr_dnn_forward_ndcg(const ultr_dnn_desc* d, const float* params, const float* wt, const float* features, int64_t n_docs,
                          const int32_t* docids, const float* labels, int32_t batch, int32_t list_size, float* scores,
                          const int32_t* topn, int32_t n_topn, float* ndcg_out, int32_t* order_out, float* masked_out,
                          float* ndcg_ws, uint32_t* counter, float* host_report, uint32_t seq, void* stream);
/* ABI 8 (additive): every metric of the reference's factory table (metrics.py:36-153, weights = None) in that ONE launch.  The list is
 * masked, validated and ranked exactly as for ultr_ndcg_report; with sl[r] the validated label at predicted rank r, n = min(topn[k], L):
 *   NDCG       as ultr_ndcg_report (the same arithmetic in the same order: the same bits)      DCG   its numerator
 *   MRR        1 / (1 + first r with sl >= 1), 0 without one                                   MAP   mean over r with sl >= 1 of hits(r) / (r + 1)
 *   ERR        sum_{r<n} rel_r prod_{q<r} (1 - rel_q) / (r + 1), rel = (2^sl - 1) / 2^max_label (the exclusive product formed directly: the
 *              reference's cumprod / (1 - rel) is NaN where rel == 1)                          ARP   sum (r + 1) sl / sum sl (0 for 0 / 0)
 *   PRECISION  count(sl >= 1) / L over the WHOLE list, as the reference's
 *   OPA        ordered_pair_accuracy: pairs (i, j) of documents with VALID labels, label_i > label_j and masked score_i > score_j
 *              (a NaN compares false), over L * L
 * Only NDCG, DCG and ERR have a cutoff; the others repeat their value per cutoff (what validation() zips with metrics_topn).
 * metric_ids [n_metrics] (1 .. ULTR_MAX_METRICS distinct ULTR_METRIC_* ids) picks the rows and their order: out [n_metrics][n_topn] batch
 * means, ws [batch][n_metrics][n_topn] per-list values.  host_report (may be NULL): a pinned, device-mapped page of >= 8 * 16 + 1 floats -
 * the n_metrics * n_topn means, then the word host_report[128] = seq.  counter as for ultr_ndcg_report (the two may share one).
 * ULTR_E_BADARG: a missing pointer, n_metrics outside 1 .. 8, an unknown or repeated id, max_label not finite, topn[k] <= 0, n_topn
 * outside 1 .. 16.  A list whose five arrays fit 64 KiB of LDS four lists at a time (list_size <= 813) takes the kernel of one wave per
 * list; a longer one takes the long-list kernel - one workgroup of 16 waves per list, its arrays in up to 160 KiB of LDS, the same
 * contract - up to ultr_metrics_max_list() documents.  ULTR_E_UNSUPPORTED: list_size beyond that. */
#define ULTR_METRIC_NDCG 0
#define ULTR_METRIC_DCG 1
#define ULTR_METRIC_MRR 2
#define ULTR_METRIC_ERR 3
#define ULTR_METRIC_MAP 4
#define ULTR_METRIC_ARP 5
#define ULTR_METRIC_PRECISION 6
#define ULTR_METRIC_OPA 7
#define ULTR_MAX_METRICS 8
int ultr_metrics_report(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                        int32_t list_size, const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics,
                        float max_label, float* out /*[n_metrics][n_topn]*/, int32_t* order_out, float* masked_out,
                        float* ws /*[batch][n_metrics][n_topn]*/, uint32_t* counter, float* host_report, uint32_t seq, void* stream);
/* ABI 8 (additive): ultr_metrics_report with the long-list kernel at EVERY list_size from 1 to ultr_metrics_max_list() - the same
 * arguments, errors and results; where ultr_metrics_report takes its one-wave kernel the two agree bit for bit (the ranks and the pair
 * count are integers, the float sums run in one wave in the same order). */
int ultr_metrics_long(const float* scores, const float* labels, const int32_t* docids, int64_t n_docs, int32_t batch,
                      int32_t list_size, const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics,
                      float max_label, float* out /*[n_metrics][n_topn]*/, int32_t* order_out, float* masked_out,
                      float* ws /*[batch][n_metrics][n_topn]*/, uint32_t* counter, float* host_report, uint32_t seq, void* stream);
/* The longest list ultr_metrics_report / ultr_metrics_long take: what 160 KiB of LDS hold of five float arrays and a validity bit per
 * document (host only, no launch). */
int32_t ultr_metrics_max_list(void);
/* validation() with those metrics as ONE host call: ultr_dnn_forward (saved = NULL), then ultr_metrics_report of its scores (lists up to
 * ultr_metrics_max_list(), as there). */
int ultr_dnn_forward_metrics(const ultr_dnn_desc* d, const float* params, const float* wt, const float* features, int64_t n_docs,
                             const int32_t* docids, const float* labels, int32_t batch, int32_t list_size, float* scores,
                             const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics, float max_label,
                             float* out, int32_t* order_out, float* masked_out, float* ws, uint32_t* counter, float* host_report,
                             uint32_t seq, void* stream);

/* ---- next row: device-side click simulation + batch assembly -------------------
 * Counterpart of ClickSimulationFeed.get_batch (click_simulation_feed.py:70-174) + PositionBiasedModel
 * (click_models.py:68-110) for a dataset RESIDENT in HBM: lists [n_queries, lmax] int32 (doc index, -1 = pad),
 * labels [n_queries, lmax] relevance.  Draws `batch` queries uniformly, samples PBM clicks
 * (exam_prob[min(l, n_exam-1)] * click_prob[min(label, n_rel-1)]), redraws lists without a click (up to
 * max_tries), and writes docids [L, B] (global doc ids, PAD = n_docs) + clicks [L, B] ready for ultr_train_step
 * with features = the resident matrix.  query_idx (may be NULL) [B] = the sampled queries.  Counter-based RNG:
 * the batch is a pure function of (seed, step).  Parity with the Python feed is distributional.
 * ABI 6: click_model = ULTR_CLICK_PBM (click_models.py:68-110) or ULTR_CLICK_CASCADE (:187-236: the same draw per position, every
 * position behind the first click reports no click) or ULTR_CLICK_UBM.  A changing bias severity (dynamic_bias_eta_change, click_simulation_feed.py:
 * 165-172) is the caller's new exam_prob table. */
#define ULTR_CLICK_PBM 0
#define ULTR_CLICK_CASCADE 1
#define ULTR_CLICK_UBM 2 /* user-browsing model (click_models.py:113-186): exam_prob = dense [n_exam][n_exam] image of the triangular
                          * table exam[rank][distance - 1] (distance to the last click; entries beyond the diagonal unused) */
/* Trust bias (additive within ABI 8; the project's own model): exam_prob = dense [2][n_exam] image, row 0
 * alpha_k, row 1 beta_k; position l, k = min(l, n_exam - 1), clicks iff u < fl(fl(alpha_k * click_prob[label]) + beta_k) - two fp32
 * roundings, no carried state.  Taken wherever a click model is: ultr_click_batch / _args, the rider of ultr_feed_train_step,
 * ultr_online_rerank_args, ultr_dbgd_interleave_args, ultr_propensity_count. */
#define ULTR_CLICK_TRUST 3
int ultr_click_batch(const int32_t* lists, const float* labels, int64_t n_queries, int32_t lmax, int64_t n_docs,
                     const float* exam_prob, int32_t n_exam, const float* click_prob, int32_t n_rel, int32_t click_model,
                     uint64_t seed, uint64_t step, int32_t batch, int32_t list_size, int32_t max_tries, int32_t* docids,
                     float* clicks, int32_t* query_idx, void* stream);
/* ABI 7: the same call from a cached argument block (the host fills it once per feed and only advances `step`), and ONE host call
 * for what `train(input_feed)` of a plugin algorithm does with a DeviceClickFeed batch: the step on the batch that is already
 * drawn (exactly ultr_train_step(a, stream)) and, behind it on the same stream, the draw of the NEXT batch into the feed's other
 * buffer (`next` may be NULL) - the draw depends on (seed, step) only, so it runs under the step's reduction / update while the host
 * is still reading this step's loss (reference: main.py:153-156 get_batch + train per step; click_simulation_feed.py:101-174).
 * ULTR_CLICK_UBM needs n_exam >= 2 (its table is rank x distance); ULTR_E_BADARG otherwise. */
typedef struct ultr_click_args {
  const int32_t* lists;
  const float* labels;
  int64_t n_queries, n_docs;
  const float* exam_prob;
  const float* click_prob;
  int32_t lmax, n_exam, n_rel, click_model;
  uint64_t seed, step;
  int32_t batch, list_size, max_tries, pad_;
  int32_t* docids;
  float* clicks;
  int32_t* query_idx;
} ultr_click_args;
int ultr_click_batch_args(const ultr_click_args* c, void* stream);
int ultr_feed_train_step(const ultr_step_args* a, const ultr_click_args* next, void* stream);

/* ---- device-resident online simulation (ultr_online.hip; additive within ABI 8) -----------------------------------------
 * Counterpart of {Stochastic,Deterministic}OnlineSimulationFeed.get_batch (stochastic_online_simulation_feed.py:96-226) for a
 * dataset RESIDENT in HBM (lists / labels as for ultr_click_batch).  Two launches around the caller's scoring forward:
 *   ultr_online_pick_args   per batch slot b: a query q drawn uniformly - among `eligible` [n_eligible] (query indexes whose
 *                           max_candidates labels do not sum to 0: the check_validation filter, precomputed by the caller) or among
 *                           all n_queries when eligible == NULL - and its first max_candidates candidates: cand_docids [M, B]
 *                           (global ids, PAD = n_docs), cand_labels [M, B] (0 at a PAD), query_idx [B] (optional).
 *   ultr_online_rerank_args per slot: list_len = 1 + the last non-PAD position; the first list_len candidates re-ranked by
 *                           `scores` [B, M] - mode ULTR_ONLINE_DETERMINISTIC: descending and stable, scores ordered as unsigned keys
 *                           (every NaN above +inf, -0 == +0); ULTR_ONLINE_STOCHASTIC: a Plackett-Luce draw at temperature tau (an
 *                           exponential race; a document whose fp32 probability exp(tau (s - max)) / sum is 0 - log p < ln 2^-150 - follows all drawn ones,
 *                           in index order) - then clicks on the first min(list_len, rank_list_size) positions of the new order
 *                           (click_model as ultr_click_batch; oracle_mode: the relevance labels), redrawn on the SAME order up to
 *                           max_redraws more times while the list has no click.  Writes docids [M, B], labels [M, B] (0 past the
 *                           cutoff) and, when non-NULL, perm [M, B] (candidate index at each rank; identity past list_len).
 * Randomness: Philox-4x32-10 keyed by (seed, step) as ultr_click_batch, own counter tags for the query pick, the race and the clicks
 * (slot, attempt, position): a batch is a pure function of (seed, step, scores).  No atomics.  max_candidates > 256: ULTR_E_BADARG. */
#define ULTR_ONLINE_DETERMINISTIC 0
#define ULTR_ONLINE_STOCHASTIC 1
typedef struct ultr_online_args {
  const int32_t* lists;
  const float* labels;
  int64_t n_queries, n_docs;
  const int32_t* eligible;
  int64_t n_eligible;
  const float* exam_prob;
  const float* click_prob;
  int32_t lmax, n_exam, n_rel, click_model;
  uint64_t seed, step;
  int32_t batch, max_candidates, rank_list_size, max_redraws;
  int32_t mode, oracle_mode;
  float tau;
  int32_t pad_;
  int32_t* cand_docids;
  float* cand_labels;
  const float* scores;
  int32_t* docids;
  float* out_labels;
  int32_t* perm;
  int32_t* query_idx;
} ultr_online_args;
int ultr_online_pick_args(const ultr_online_args* a, void* stream);
int ultr_online_rerank_args(const ultr_online_args* a, void* stream);

/* ---- DBGD / MGD: weight-perturbing online learners (ultr_dbgd.hip; additive within ABI 8) ---------------------------------
 * Counterpart of DBGD.train / MGD.train (dbgd.py:125-330, mgd.py:86-232) and TeamDraftInterleaving (team_draft_interleave.py).
 * R = n_rankers candidates (DBGD 1, MGD ranker_num); ranker 0 is the current model.  A step, on one stream:
 *   ultr_dbgd_noise_args       noise [R, P]: per Linear parameter F.normalize(N(0, 1), dim = 0) - per input column of a weight
 *                              (over `out`), over a whole bias; the [1, in] scorer row becomes sign(z) - and 0 on the LayerNorm
 *                              entries; cand_params [R, cand_stride] = params + noise_rate * noise.  noise_in [R, P] (optional): the raw
 *                              normals instead of the Philox draw (entries of LayerNorm parameters unused).
 *   the caller's R + 1 forwards (ultr_dnn_forward with saved = NULL, ultr_dnn_build_wt before each candidate's) into
 *   scores [R + 1, B, L]: L = max_candidates with need_interleave, rank_list_size without.
 *   ultr_dbgd_interleave_args  (need_interleave) per list: list_len = 1 + the last non-PAD position (docids [M, B], PAD = n_docs);
 *                              each ranker's order of the first list_len candidates (mode as ultr_online_rerank_args: the stable
 *                              descending sort or the Plackett-Luce race at tau); the team-draft multileave (the agreed prefix is
 *                              team -1, then a fresh shuffle of the rankers every R + 1 picks); clicks (click_model as
 *                              ultr_click_batch) on labels [M, B] in the multileaved order, first min(list_len, rank_list_size)
 *                              positions, redrawn up to max_redraws more times while the list has none; winners [B, R + 1] =
 *                              clicks of team r / (clicks of all teams + 1e-7).  Optional outputs [M, B]: interleaved (candidate
 *                              index, -1 past list_len), teams (-1 agreed prefix, -2 past list_len), clicks (0 past the cutoff);
 *                              loss_scores [B, rank_list_size] = ranker 0's first rank_list_size scores (for ultr_ndcg).
 *                              Optional injected draws: shuffles_in [B, M, R + 1] (the ranker order of round t of list b) and
 *                              clicks_in [M, B] (the clicks; no redraw).
 *   the caller's ultr_ndcg (docids = NULL: PADs unmasked, as dbgd.py:138-149) of NDCG@rank_list_size into ndcg [R + 1]:
 *                              ndcg[0] of the current model (the loss is 1 - ndcg[0]); without interleaving every ranker's.
 *   ultr_dbgd_grad_args        grads [P + ultr_step_tail_floats(max_candidates)] = -sum_r c_r noise_r (the update steps TOWARD the
 *                              winners), c_r = mean_b winners[b, r] (need_interleave) or the mean of the reference's batch-level
 *                              winners ceil(ndcg_r - ndcg_0) / (sum + 1e-9); step tail [0] = the loss, [1] = 1; the sum-of-squares
 *                              partials at the head of bwd_ws.  Then ultr_apply_update (algo ULTR_ALGO_DBGD, l2_loss = 0,
 *                              list_size = max_candidates).
 * Randomness: Philox-4x32-10 keyed by (seed, step), own counter tags for the noise (element, ranker), the race (list, ranker,
 * position), the shuffles (list, round) and the clicks (list, attempt, position).  No atomics.
 * ULTR_E_BADARG: max_candidates > 256, n_rankers + 1 > 16, rank_list_size > max_candidates, n_params != the desc's. */
#define ULTR_DBGD_MAX_M 256
#define ULTR_DBGD_MAX_RANKERS 16 /* R + 1 */
typedef struct ultr_dbgd_args {
  const ultr_dnn_desc* desc;
  int64_t n_params;
  int32_t n_rankers, batch, max_candidates, rank_list_size;
  int32_t need_interleave, mode, max_redraws, click_model;
  int32_t n_exam, n_rel;
  float noise_rate, tau;
  uint64_t seed, step;
  const float* params;
  const float* noise_in;
  float* noise;
  float* cand_params;
  int64_t cand_stride; /* floats from one candidate vector to the next (0: n_params); a multiple of 4 keeps each 16-byte aligned */
  const float* scores;
  const int32_t* docids;
  int64_t n_docs;
  const float* labels;
  const float* exam_prob;
  const float* click_prob;
  const int32_t* shuffles_in;
  const float* clicks_in;
  float* winners;
  int32_t* interleaved;
  int32_t* teams;
  float* clicks;
  float* loss_scores;
  const float* ndcg;
  float* grads;
  void* bwd_ws;
} ultr_dbgd_args;
int ultr_dbgd_noise_args(const ultr_dbgd_args* a, void* stream);
int ultr_dbgd_interleave_args(const ultr_dbgd_args* a, void* stream);
int ultr_dbgd_grad_args(const ultr_dbgd_args* a, void* stream);

/* ---- NSGD: DBGD / MGD with null-space exploration (ultr_nsgd.hip; additive within ABI 8) ----------------------------------
 * Counterpart of NSGD.train (nsgd.py): MGD's step with its noise launch replaced and one launch added.  `dbgd` points at the
 * step's ultr_dbgd_args (desc, n_params, n_rankers R, seed, step, params, noise, cand_params, cand_stride, noise_rate,
 * need_interleave, batch, winners, ndcg); memory [R, n_params] holds the last losing directions (0 outside the Linear entries).
 * A Linear tensor t is a weight [out, in] or a bias [out] of the flat DNN vector.  A step, on one stream:
 *   ultr_nsgd_noise_args   noise [R, P]: per Linear tensor t and ranker r, u_{t,r} = z / sqrt(max(sum z^2, 1e-12)) with
 *                          z = P_t z_{t,r}, z_{t,r} Philox normals (Box-Muller, own tag) and P_t the orthogonal projection onto the
 *                          complement of memory's rows restricted to t (exactly-zero rows are empty slots; rows the fp64 pivoted
 *                          Cholesky of their Gram matrix finds dependent are dropped); u = 0 when the kept rows span t; a bias of
 *                          one entry skips the projection (+-1).  0 on the LayerNorm entries.  cand_params [R, cand_stride] =
 *                          params + noise_rate * noise.  Four launches (partial dot products; their fixed-order reduction and the
 *                          solve, one workgroup per tensor; projection and partial sums of squares; normalization and the
 *                          candidates): a step is a pure function of (seed, step, params, memory), independent of the launch
 *                          geometry.  Optional: normals_in [R, P] replaces the Philox draw; unit_noise_in [R, P] replaces the whole
 *                          law (noise = unit_noise_in on the Linear entries; one launch).
 *   then DBGD's forwards, ultr_dbgd_interleave_args / ultr_ndcg, ultr_dbgd_grad_args and ultr_apply_update, unchanged.
 *   ultr_nsgd_memory_args  after the winners (need_interleave) or the R + 1 NDCGs (without): memory row r = noise_r on the Linear
 *                          entries if ranker r + 1 lost, else 0.  Lost: with interleaving, winners[b, r + 1] = 0 for every list b;
 *                          without, the reference's batch-level winners w = ceil(ndcg_a - ndcg_0) / (sum + 1e-9) sum to 0 (then
 *                          every row stores its noise, else every row is zeroed).
 * ws: ultr_nsgd_workspace_bytes(desc, n_rankers) bytes, 8-byte aligned.  No atomics.
 * ULTR_E_BADARG: as ultr_dbgd_noise_args, or a missing memory / ws. */
typedef struct ultr_nsgd_args {
  const ultr_dbgd_args* dbgd;
  float* memory;
  const float* normals_in;
  const float* unit_noise_in;
  void* ws;
} ultr_nsgd_args;
int64_t ultr_nsgd_workspace_bytes(const ultr_dnn_desc* desc, int32_t n_rankers);
int ultr_nsgd_noise_args(const ultr_nsgd_args* a, void* stream);
int ultr_nsgd_memory_args(const ultr_nsgd_args* a, void* stream);

/* ---- propensity estimation from randomized click sessions (ultr_propensity.hip; additive within ABI 8) ------------------------
 * Counterpart of the session loop of RandomizedPropensityEstimator.estimateParametersFromModel (propensity_estimator.py:95-118):
 * n_sessions times, pick a label list uniformly, shuffle it uniformly, sample clicks on the shuffled list with the click model
 * (no redraw of click-less lists), and add every click to click_count[len - 1][position].  The table is ADDED to, never cleared:
 * the caller zeroes it once and may split the sessions over any number of calls.
 *   labels  [n_queries][lmax] relevance, row q valid in [0, lengths[q]);  lengths [n_queries], 0 .. lmax
 *   exam_prob / n_exam / click_prob / n_rel / click_model: as ultr_click_args (ULTR_CLICK_UBM: dense [n_exam][n_exam] image)
 *   click_count [lmax][lmax] 64-bit counters, row = list length - 1, column = position
 * Session s (first_session <= s < first_session + n_sessions) is a pure function of (seed, s): Philox under ultr_click_batch's key
 * with step = 0, counters (lo32(s), hi32(s), g, tag).  Query: q = min((int64)((double)u01(word 0 of (.., 0xFFFFFFFF, query tag)) *
 * n_queries), n_queries - 1), n = lengths[q].  Shuffle: position l < n gets the 32-bit word l & 3 of (.., l >> 2, shuffle tag) as its
 * key; the label at rank r is the one whose key is the r-th largest (ties by index).  Clicks: the uniform of rank r is u01(word
 * r & 3 of (.., r >> 2, click tag)), the decision ultr_click_batch's for a list of n positions.  A session with n == 0 counts nothing.
 * Persistent workgroups accumulate in a 32-bit LDS histogram and flush once with 64-bit integer atomic adds: the table is
 * independent of the launch geometry and of the order of the adds (bit-reproducible).  The parity with the reference's Python
 * random stream is distributional.
 * ULTR_E_BADARG: a missing pointer, n_queries / lmax / n_exam / n_rel <= 0, n_sessions < 0, an unknown click model, ULTR_CLICK_UBM
 * with n_exam < 2.  ULTR_E_UNSUPPORTED: lmax > ULTR_PROPENSITY_MAX_L.  Neither launches anything; n_sessions == 0 is a no-op. */
#define ULTR_PROPENSITY_MAX_L 128
typedef struct ultr_propensity_args {
  const float* labels;
  const int32_t* lengths;
  int64_t n_queries;
  int32_t lmax;
  const float* exam_prob;
  int32_t n_exam;
  const float* click_prob;
  int32_t n_rel, click_model;
  uint64_t seed, first_session;
  int64_t n_sessions;
  unsigned long long* click_count;
} ultr_propensity_args;
int ultr_propensity_count(const ultr_propensity_args* a, void* stream);

/* ---- per-click weights of a click model with a click history (ultr_history_pw.hip; additive within ABI 8) ---------------------
 * Counterpart of OraclePropensityEstimator.getPropensityForOneList on a user-browsing model (propensity_estimator.py:149-180,
 * click_models.py:151-162), whose weight at a position depends on where the previous click of the same list was.
 *   labels [L, B] clicks (> 0 = clicked);  table [L][L] row-major: row = position, column = position of the last click before it + 1
 *   (column 0: no click so far; entries beyond the diagonal are never read);  pw_out [B, L].
 * With last(b, l) = the largest l' < l with labels[l', b] > 0, or -1:
 *   pw_out[b, l] = (all_positions || labels[l, b] > 0) ? table[l * L + last(b, l) + 1] : 0
 * all_positions = 0: IPWrank (getPropensityForOneList(click_list)); 1: PRSrank (use_non_clicked_data=True).  The table is the
 * host's (OraclePropensityEstimator.weight_table: the model's own expression per entry, rounded to float32 once), the launch only
 * looks up: the weights are the reference's bit for bit.  Lists of up to 32 positions are packed 8 / 4 / 2 to a wavefront.  No
 * atomics, no dependence on the launch geometry, any list_size >= 1.
 * ULTR_E_BADARG: a NULL argument block or pointer, batch <= 0, list_size <= 0, all_positions outside {0, 1}.  Launches nothing then. */
typedef struct ultr_history_pw_args {
  const float* labels;
  const float* table;
  float* pw_out;
  int32_t batch, list_size, all_positions, pad_;
} ultr_history_pw_args;
int ultr_history_pw(const ultr_history_pw_args* a, void* stream);

/* ---- a whole validation / test set from a RESIDENT dataset (ultr_eval.hip; additive within ABI 8) -----------------------------------
 * Counterpart of the driver's evaluation loop (main.py:85-227 validate, :230-292 test): DirectLabelFeed.get_next_batch per batch
 * (direct_label_feed.py:36-47), validation() per batch, utils.merge_Summary at the end (data_utils.py:501-514) - for a dataset
 * RESIDENT in HBM (lists / labels as for ultr_click_batch).
 *   ultr_eval_pick        the sequential sibling of ultr_online_pick_args: queries start .. start + batch - 1 and positions
 *                         l < list_size: docids_out [L, B] = the list entry, or n_docs (PAD) where the entry is < 0 or l >= lmax;
 *                         labels_out [L, B] = the label, 0 at a PAD (prepare_true_labels_with_index, direct_label_feed.py:19-23);
 *                         query_idx_out [B] (may be NULL) = start + b.  One wavefront per slot, four slots per workgroup; ANY
 *                         list_size >= 1 (no 256 cap: validation lists can be long).
 *                         ULTR_E_BADARG: a missing pointer (query_idx_out excepted), n_queries / lmax <= 0, n_docs outside 0 .. 2^31 - 1,
 *                         start < 0, batch <= 0, start + batch > n_queries, list_size <= 0.  Launches nothing then.
 *   ultr_eval_accumulate  merge_Summary operation for operation in double: acc[i] += (double)batch_means[i] * (double)batch for
 *                         i < n_values, acc[n_values] += batch; acc [n_values + 1] doubles on the device.  flags: ULTR_EVAL_RESET - the
 *                         accumulator counts as zero before the add (it need not be cleared); ULTR_EVAL_FINISH - after the add,
 *                         host_report[i] = acc[i] / max(1e-7, acc[n_values]) (IEEE round-to-nearest), host_report[128] = acc[n_values],
 *                         then the 32-bit word behind 129 doubles (byte offset ULTR_EVAL_SEQ_BYTE) = seq, ordered behind the values as
 *                         ultr_metrics_report orders its report.  host_report: pinned, device-mapped, >= ULTR_EVAL_SEQ_BYTE + 4 bytes
 *                         (required with ULTR_EVAL_FINISH).  One workgroup, one thread per value: no reduction, no atomics.
 *                         ULTR_E_BADARG: a missing pointer, n_values outside 1 .. 128, batch <= 0, unknown flag bits.
 *   ultr_dnn_eval_set     the whole set from ONE host call: per chunk of `batch` queries (the last one short) ultr_eval_pick into
 *                         docids_ws / labels_ws [L, batch], ultr_dnn_forward_metrics of the chunk (host report NULL; topn, metric_ids,
 *                         max_label, out, order_out, masked_out, ws, counter as there, sized for `batch` lists) and
 *                         ultr_eval_accumulate of `out` (n_values = n_metrics * n_topn) - ULTR_EVAL_RESET on the first chunk,
 *                         ULTR_EVAL_FINISH on the last.  scores_all [n_queries, L] / per_query [n_queries, n_metrics, n_topn] (either
 *                         may be NULL): every chunk's scores / per-list metric values written straight to their offset; otherwise
 *                         they go to scores_ws [batch, L] / ws and only the last chunk's remain.  The launches of a chunk are exactly
 *                         the ones validation() issues for that batch: the merged figures are the per-batch loop's, bit for bit.
 *                         list_size up to ultr_metrics_max_list(), as ultr_metrics_report (ULTR_E_UNSUPPORTED beyond).
 *                         Does not synchronise, does not allocate, stops at the first non-zero return. */
#define ULTR_EVAL_RESET 1
#define ULTR_EVAL_FINISH 2
#define ULTR_EVAL_SEQ_BYTE (129 * 8)
int ultr_eval_pick(const int32_t* lists, const float* labels, int64_t n_queries, int32_t lmax, int64_t n_docs, int64_t start,
                   int32_t batch, int32_t list_size, int32_t* docids_out, float* labels_out, int32_t* query_idx_out, void* stream);
int ultr_eval_accumulate(const float* batch_means, int32_t n_values, int32_t batch, double* acc, int32_t flags, double* host_report,
                         uint32_t seq, void* stream);
int ultr_dnn_eval_set(const ultr_dnn_desc* d, const float* params, const float* wt, const float* features, int64_t n_docs,
                      const int32_t* lists, const float* labels, int64_t n_queries, int32_t lmax, int32_t batch, int32_t list_size,
                      const int32_t* topn, int32_t n_topn, const int32_t* metric_ids, int32_t n_metrics, float max_label,
                      int32_t* docids_ws, float* labels_ws, float* scores_ws, float* out, int32_t* order_out, float* masked_out, float* ws,
                      uint32_t* counter, float* scores_all, float* per_query, double* acc, double* host_report, uint32_t seq,
                      void* stream);

/* ---- e: data-parallel gradient exchange over xGMI -----------------------------
 * No reference counterpart: the reference is single-process.  One process per GPU; queries shard across ranks,
 * parameters / optimizer / EM state are replicated, and ONE sum per step of the flat vector
 * grads[P + tail] (what ultr_dnn_backward / ultr_train_step(skip_update) leave) makes every rank's update identical.
 * ultr_comm_allreduce is that sum as ONE kernel: every rank publishes its vector into a fine-grained exchange
 * buffer mapped by all peers (hipIpc handles), reads every peer's copy over xGMI, adds them in rank order (bitwise
 * identical results on all ranks, deterministic) and leaves the sum-of-squares partials of the reduced gradient
 * where ultr_apply_update expects them (so no ultr_grad_sumsq pass).  Waits are bounded; a timeout is reported by
 * ultr_comm_status (ULTR_E_COMM_TIMEOUT) and the caller falls back to its collective library.
 * The exchange buffer is the one allocation this library makes (it must be IPC-exportable fine-grained memory);
 * handles are ULTR_COMM_HANDLE_BYTES opaque bytes the caller moves between processes (parallel.py: all_gather).
 *   create(rank, world, n_floats)  n_floats >= P + tail; zeroed flags, device-synchronising
 *   export(handle_out) / import(peer, handle)   once per peer, before the first all-reduce
 *   allreduce(step, src, n, n_params, out, sumsq_ws, sumsq_parts, stream)   step = 0, 1, 2, ... in lockstep on all
 *       ranks; src/out [n] local device vectors (may alias); sumsq_ws = head of bwd_ws, sumsq_parts =
 *       ceil((P + tail) / 64) as for ultr_grad_sumsq.  world == 1 degenerates to copy + partials. */
#define ULTR_COMM_MAX_WORLD 8
#define ULTR_COMM_HANDLE_BYTES 64
typedef struct ultr_comm ultr_comm;
int ultr_comm_create(int32_t rank, int32_t world, int64_t n_floats, ultr_comm** out);
int ultr_comm_export(ultr_comm* c, void* handle_out);
int ultr_comm_import(ultr_comm* c, int32_t peer, const void* handle);
int ultr_comm_allreduce(ultr_comm* c, uint64_t step, const float* src, int64_t n, int64_t n_params, float* out,
                        void* sumsq_ws, int32_t sumsq_parts, void* stream);
/* synchronises `stream`, then 0 or ULTR_E_COMM_TIMEOUT */
int ultr_comm_status(ultr_comm* c, void* stream);
int ultr_comm_destroy(ultr_comm* c);

/* ---- measurement hooks (bench.py only; not part of the reference's interface) ----------
 * Per-kernel timers: an armed kernel is launched with a start and a stop event taken from its OWN dispatch
 * packet (hipExtLaunchKernelGGL), i.e. the duration rocprofv3 --kernel-trace reports, without marker packets
 * on the stream.  kernel ids: 0 forward, 1 loss, 2 backward (dgrad chain), 3 weight gradients, 4 gradient
 * reduction, 5 update.  enable(mask, n) arms up to n samples for the kernels in mask (0 disarms);
 * set_stride(k) times only every k-th launch of an armed kernel; collect() synchronises the recorded events,
 * returns per-kernel total milliseconds and sample counts in arrays of 8, and rearms. */
int ultr_prof_enable(uint32_t kernel_mask, int32_t max_samples);
int ultr_prof_set_stride(int32_t every_nth_launch);
int ultr_prof_collect(double* total_ms, int64_t* counts);

/* The ULTR_* tuning knobs (README.md) are read from the environment once, at first use; this re-reads them (tests and the
 * A/B tools flip knobs inside one process). */
int ultr_config_reload(void);

#ifdef __cplusplus
}
#endif
#endif /* ULTR_HIP_H */
