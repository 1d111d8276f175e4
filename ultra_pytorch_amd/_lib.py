"""ctypes binding of libultr_hip.so (the C ABI declared in include/ultr_hip.h).

The reference-side stub shown in INTEGRATION.md is this file minus the conveniences.
Fails loudly when the library is missing — there is no fallback path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libultr_hip.so")

ULTR_MAX_HIDDEN = 7
COMM_HANDLE_BYTES, COMM_MAX_WORLD = 64, 8
ACT = {"elu": 0, "relu": 1, "tanh": 2, "sigmoid": 3}  # base_ranking_model.py:63-69 ("selu" raises in the reference)
ATTN_DTYPE = {"fp32": 0, "fp16": 1}
ALGO_SOFTMAX, ALGO_DLA, ALGO_PAIRDEBIAS, ALGO_LAMBDARANK, ALGO_REGEM, ALGO_PRS, ALGO_PDGD, ALGO_DBGD = 0, 1, 2, 3, 4, 5, 6, 7
ALGO_TWOTOWER = 9  # (8 is no algorithm: include/ultr_hip.h)
TWOTOWER_SUM, TWOTOWER_MASK = 1, 2  # ultr_twotower_loss's combination; bits of ultr_update_desc::logits_to_prob
ALGO_PLRANK = 11  # (10 is no algorithm either)
PLRANK_GAIN = {"linear": 0, "exp2": 1}  # ULTR_PLRANK_GAIN_*
PLRANK_MAX_SAMPLES = 4095


def plrank_pack(cutoff, n_samples, gain):
    """ULTR_PLRANK_PACK: what ultr_update_desc::logits_to_prob carries for a PLRank step (bits 0-11 cutoff, 12-23 samples, 24 exp2)."""
    return min(int(cutoff), 4095) | (int(n_samples) << 12) | (PLRANK_GAIN[gain] << 24)
ALGO_AFFINE = 12
AFFINE_MASK = 1  # ULTR_AFFINE_MASK: bit 0 of ultr_update_desc::logits_to_prob of an AffineRank step
OPT_ADAGRAD, OPT_SGD, OPT_ADAM = 0, 1, 2
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8  # include/ultr_hip.h: ULTR_ADAM_*

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class DnnDesc(ctypes.Structure):
    _fields_ = [("feature_size", c_i32), ("n_hidden", c_i32), ("hidden", c_i32 * ULTR_MAX_HIDDEN), ("activation", c_i32),
                ("flags", c_i32)]


class DnnRouteInfo(ctypes.Structure):  # ultr_dnn_route_info (ultr_dnn_route)
    _fields_ = [("fused_waves", c_i32), ("fwd", c_i32), ("fwd_rows", c_i32), ("bwd", c_i32), ("bwd_rows", c_i32), ("loss", c_i32),
                ("wg_split_half", c_i32), ("reserved", c_i32 * 5)]


DNN_CALLS = ("eval", "step_softmax", "step_dscores")  # include/ultr_hip.h: ultr_dnn_route_call
DNN_FAMILIES = ("none", "tile", "tile2", "wide", "per_layer", "fused", "unsupported")  # ultr_dnn_family
DNN_LOSS_PLACES = ("none", "launch", "prologue", "fused")  # ultr_dnn_loss_place
# ULTR_DNN_OP_*: what a call passes (ultr_dnn_route_operands); a weight copy off a 16-byte boundary counts as absent
DNN_OPERANDS = {"params16": 1, "features16": 2, "wt": 4, "wt16": 8, "dscores": 16}
DNN_OP_ALL = 31

MODEL_FP32_PRODUCTS = 1  # ultr_dnn_desc / ultr_setrank_desc ::flags (include/ultr_hip.h, ABI 6)
MODEL_SR_STREAM_BWD = 2  # ultr_setrank_desc::flags: the streaming attention backward beyond the one-pass kernels' list bounds
ABI_VERSION = 8          # include/ultr_hip.h: ULTR_ABI_VERSION - load() refuses a library that reports another one


class UpdateDesc(ctypes.Structure):
    _fields_ = [("algo", c_i32), ("optimizer", c_i32), ("list_size", c_i32), ("logits_to_prob", c_i32),
                ("n_params", c_i64), ("learning_rate", c_f32), ("max_gradient_norm", c_f32), ("adagrad_eps", c_f32),
                ("ranker_loss_weight", c_f32), ("propensity_learning_rate", c_f32), ("em_step_size", c_f32),
                ("regulation_p", c_f32), ("l2_loss", c_f32), ("guard", c_vp), ("host_scalars", c_vp),
                ("seq", ctypes.c_uint32), ("adam_t", ctypes.c_uint32), ("range_flag", c_vp)]


class ClickArgs(ctypes.Structure):  # ultr_click_args (ABI 7)
    _fields_ = [("lists", c_vp), ("labels", c_vp), ("n_queries", c_i64), ("n_docs", c_i64), ("exam_prob", c_vp), ("click_prob", c_vp),
                ("lmax", c_i32), ("n_exam", c_i32), ("n_rel", c_i32), ("click_model", c_i32), ("seed", ctypes.c_uint64),
                ("step", ctypes.c_uint64), ("batch", c_i32), ("list_size", c_i32), ("max_tries", c_i32), ("pad_", c_i32),
                ("docids", c_vp), ("clicks", c_vp), ("query_idx", c_vp)]


class OnlineArgs(ctypes.Structure):  # ultr_online_args (ultr_online_pick_args / ultr_online_rerank_args)
    _fields_ = [("lists", c_vp), ("labels", c_vp), ("n_queries", c_i64), ("n_docs", c_i64), ("eligible", c_vp), ("n_eligible", c_i64),
                ("exam_prob", c_vp), ("click_prob", c_vp), ("lmax", c_i32), ("n_exam", c_i32), ("n_rel", c_i32), ("click_model", c_i32),
                ("seed", ctypes.c_uint64), ("step", ctypes.c_uint64), ("batch", c_i32), ("max_candidates", c_i32),
                ("rank_list_size", c_i32), ("max_redraws", c_i32), ("mode", c_i32), ("oracle_mode", c_i32), ("tau", c_f32),
                ("pad_", c_i32), ("cand_docids", c_vp), ("cand_labels", c_vp), ("scores", c_vp), ("docids", c_vp),
                ("out_labels", c_vp), ("perm", c_vp), ("query_idx", c_vp)]


ONLINE_DETERMINISTIC, ONLINE_STOCHASTIC = 0, 1  # ultr_online_args::mode


class DbgdArgs(ctypes.Structure):  # ultr_dbgd_args (ultr_dbgd_noise_args / ultr_dbgd_interleave_args / ultr_dbgd_grad_args)
    _fields_ = [("desc", ctypes.POINTER(DnnDesc)), ("n_params", c_i64), ("n_rankers", c_i32), ("batch", c_i32),
                ("max_candidates", c_i32), ("rank_list_size", c_i32), ("need_interleave", c_i32), ("mode", c_i32),
                ("max_redraws", c_i32), ("click_model", c_i32), ("n_exam", c_i32), ("n_rel", c_i32), ("noise_rate", c_f32),
                ("tau", c_f32), ("seed", ctypes.c_uint64), ("step", ctypes.c_uint64), ("params", c_vp), ("noise_in", c_vp),
                ("noise", c_vp), ("cand_params", c_vp), ("cand_stride", c_i64), ("scores", c_vp), ("docids", c_vp), ("n_docs", c_i64), ("labels", c_vp),
                ("exam_prob", c_vp), ("click_prob", c_vp), ("shuffles_in", c_vp), ("clicks_in", c_vp), ("winners", c_vp),
                ("interleaved", c_vp), ("teams", c_vp), ("clicks", c_vp), ("loss_scores", c_vp), ("ndcg", c_vp), ("grads", c_vp),
                ("bwd_ws", c_vp)]


DBGD_MAX_M, DBGD_MAX_RANKERS = 256, 16  # include/ultr_hip.h: ULTR_DBGD_MAX_M, ULTR_DBGD_MAX_RANKERS (R + 1)


class NsgdArgs(ctypes.Structure):  # ultr_nsgd_args (ultr_nsgd_noise_args / ultr_nsgd_memory_args)
    _fields_ = [("dbgd", ctypes.POINTER(DbgdArgs)), ("memory", c_vp), ("normals_in", c_vp), ("unit_noise_in", c_vp), ("ws", c_vp)]


class PropensityArgs(ctypes.Structure):  # ultr_propensity_args (ultr_propensity_count)
    _fields_ = [("labels", c_vp), ("lengths", c_vp), ("n_queries", c_i64), ("lmax", c_i32), ("exam_prob", c_vp), ("n_exam", c_i32),
                ("click_prob", c_vp), ("n_rel", c_i32), ("click_model", c_i32), ("seed", ctypes.c_uint64),
                ("first_session", ctypes.c_uint64), ("n_sessions", c_i64), ("click_count", c_vp)]


class HistoryPwArgs(ctypes.Structure):  # ultr_history_pw_args (ultr_history_pw)
    _fields_ = [("labels", c_vp), ("table", c_vp), ("pw_out", c_vp), ("batch", c_i32), ("list_size", c_i32), ("all_positions", c_i32),
                ("pad_", c_i32)]


PROPENSITY_MAX_L = 128  # include/ultr_hip.h: ULTR_PROPENSITY_MAX_L
EVAL_RESET, EVAL_FINISH, EVAL_SEQ_BYTE = 1, 2, 129 * 8  # include/ultr_hip.h: ULTR_EVAL_*


class SetRankDesc(ctypes.Structure):
    _fields_ = [("feature_size", c_i32), ("d_model", c_i32), ("num_heads", c_i32), ("num_layers", c_i32), ("dff", c_i32),
                ("attention_dtype", c_i32), ("flags", c_i32)]


# include/ultr_hip.h: ultr_setrank_attn_path_id - the attention kernel family a shape takes (ultr_setrank_attn_path)
SR_ATTN_PATHS = ("scalar", "mfma", "f16", "split_half", "long_mfma", "long_scalar")


class SetRankRouteInfo(ctypes.Structure):  # ultr_setrank_route_info (ultr_setrank_route)
    _fields_ = [("embed", c_i32), ("block", c_i32), ("head_rides", c_i32), ("skip_out1", c_i32), ("bwd_head", c_i32),
                ("bwd_blocks", c_i32), ("bwd_embed", c_i32), ("rows_per_tile", c_i32), ("tiles", c_i32), ("workgroups", c_i32),
                ("block_rows", c_i32), ("embed_rows", c_i32), ("wgrad_split", c_i32), ("reserved", c_i32 * 3)]


SR_BLOCK_SEPARATE, SR_BLOCK_ROUND5, SR_BLOCK_PERSISTENT = 0, 1, 2  # ultr_setrank_route_info::block


class SetRankDropout(ctypes.Structure):  # ultr_setrank_dropout
    _fields_ = [("rate", c_f32), ("seed", ctypes.c_uint64), ("step", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("scratch", c_vp),
                ("scratch_bytes", c_i64)]


class DlcmDesc(ctypes.Structure):  # ultr_dlcm_desc
    _fields_ = [("feature_size", c_i32), ("hidden_size", c_i32), ("num_heads", c_i32)]


class GsfDesc(ctypes.Structure):  # ultr_gsf_desc
    _fields_ = [("feature_size", c_i32), ("group_size", c_i32), ("n_hidden", c_i32), ("hidden", c_i32 * ULTR_MAX_HIDDEN),
                ("activation", c_i32)]


GSF_MAX_GROUP = 8  # csrc/ultr_gsf_plan.h: documents per group the kernels take


class StepArgs(ctypes.Structure):
    _fields_ = [("desc", ctypes.POINTER(DnnDesc)), ("upd", ctypes.POINTER(UpdateDesc)), ("params", c_vp), ("wt", c_vp),
                ("state", c_vp), ("aux", c_vp), ("features", c_vp), ("docids", c_vp), ("labels", c_vp), ("pw", c_vp),
                ("ipw_table", c_vp), ("scores", c_vp), ("dscores", c_vp), ("saved", c_vp), ("loss_ws", c_vp),
                ("bwd_ws", c_vp), ("grads", c_vp), ("scalars", c_vp), ("n_docs", c_i64), ("n_ipw", c_i32),
                ("batch", c_i32), ("list_size", c_i32), ("batch_total", c_i32), ("skip_update", c_i32), ("sigma", c_f32),
                ("uniforms", c_vp), ("rng_seed", ctypes.c_uint64), ("rng_step", ctypes.c_uint64),
                ("comm", c_vp), ("comm_step", ctypes.c_uint64)]


# name -> (restype, argtypes); must list EVERY symbol include/ultr_hip.h declares
SIGNATURES = {
    "ultr_abi_version": (c_i32, []),
    "ultr_dnn_param_count": (c_i64, [ctypes.POINTER(DnnDesc)]),
    "ultr_dnn_param_offsets": (c_i32, [ctypes.POINTER(DnnDesc), ctypes.POINTER(c_i64)]),
    "ultr_dnn_saved_bytes": (c_i64, [ctypes.POINTER(DnnDesc), c_i64]),
    "ultr_dnn_bwd_workspace_bytes": (c_i64, [ctypes.POINTER(DnnDesc), c_i64]),
    "ultr_step_tail_floats": (c_i64, [c_i32]),
    "ultr_loss_workspace_bytes": (c_i64, [c_i64, c_i32]),
    "ultr_loss_part_count": (c_i64, [c_i64]),
    "ultr_loss_lds_bytes": (c_i64, [c_i32, c_i32]),
    "ultr_dnn_forward": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_dnn_wt_floats": (c_i64, [ctypes.POINTER(DnnDesc)]),
    "ultr_dnn_build_wt": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp]),
    "ultr_dnn_wt_range": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp]),
    "ultr_dnn_forward_tile_rows": (c_i32, [ctypes.POINTER(DnnDesc), c_i64, c_i32]),
    "ultr_dnn_backward_tile_rows": (c_i32, [ctypes.POINTER(DnnDesc), c_i64]),
    "ultr_fused_fb_waves": (c_i32, [ctypes.POINTER(DnnDesc), c_i32, c_i32]),
    "ultr_dnn_route": (c_i32, [ctypes.POINTER(DnnDesc), c_i32, c_i32, c_i64, c_i32, ctypes.POINTER(DnnRouteInfo)]),
    "ultr_dnn_route_operands": (c_i32, [ctypes.POINTER(DnnDesc), c_i32, c_i32, c_i64, c_i32, ctypes.c_uint32,
                                        ctypes.POINTER(DnnRouteInfo)]),
    "ultr_dnn_backward": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp]),
    "ultr_dnn_backward_softmax": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                          c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "ultr_grad_sumsq": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp]),
    "ultr_softmax_ce": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_dla_loss": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_pairdebias_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_lambdarank_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_prs_loss": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_prs_loss_pw": (c_i32, [c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_pdgd_loss": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_f32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_loss_long_lds_bytes": (c_i64, [c_i32, c_i32]),
    "ultr_loss_long_max_list": (c_i32, [c_i32]),
    "ultr_pairdebias_loss_long": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_lambdarank_loss_long": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_prs_loss_long": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_prs_loss_pw_long": (c_i32, [c_vp, c_vp, c_vp, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_regem_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, ctypes.c_uint64, ctypes.c_uint64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_twotower_loss": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_plrank_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_i32, ctypes.c_uint64, ctypes.c_uint64,
                                 c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_affine_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_setrank_param_count": (c_i64, [ctypes.POINTER(SetRankDesc)]),
    "ultr_setrank_saved_bytes": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_workspace_bytes": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_range_flag_offset": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_forward": (c_i32, [ctypes.POINTER(SetRankDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "ultr_setrank_backward": (c_i32, [ctypes.POINTER(SetRankDesc), c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp,
                                      c_vp]),
    "ultr_setrank_score_bytes": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_score_range_flag_offset": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_score": (c_i32, [ctypes.POINTER(SetRankDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "ultr_setrank_attn_path": (c_i32, [ctypes.POINTER(SetRankDesc), c_i32, c_i32]),
    "ultr_setrank_route": (c_i32, [ctypes.POINTER(SetRankDesc), c_i32, c_i32, c_i32, ctypes.POINTER(SetRankRouteInfo)]),
    "ultr_setrank_dropout_workspace_bytes": (c_i64, [ctypes.POINTER(SetRankDesc), c_i64]),
    "ultr_setrank_forward_dropout": (c_i32, [ctypes.POINTER(SetRankDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp,
                                             ctypes.POINTER(SetRankDropout), c_vp]),
    "ultr_setrank_backward_dropout": (c_i32, [ctypes.POINTER(SetRankDesc), c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp,
                                              ctypes.POINTER(SetRankDropout), c_vp]),
    "ultr_dlcm_param_offsets": (c_i32, [ctypes.POINTER(DlcmDesc), ctypes.POINTER(c_i64)]),
    "ultr_dlcm_saved_bytes": (c_i64, [ctypes.POINTER(DlcmDesc), c_i64]),
    "ultr_dlcm_score_bytes": (c_i64, [ctypes.POINTER(DlcmDesc), c_i64]),
    "ultr_dlcm_workspace_bytes": (c_i64, [ctypes.POINTER(DlcmDesc), c_i32, c_i32]),
    "ultr_dlcm_forward": (c_i32, [ctypes.POINTER(DlcmDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_dlcm_backward": (c_i32, [ctypes.POINTER(DlcmDesc), c_vp, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp,
                                   c_vp]),
    "ultr_gsf_param_count": (c_i64, [ctypes.POINTER(GsfDesc)]),
    "ultr_gsf_param_offsets": (c_i32, [ctypes.POINTER(GsfDesc), ctypes.POINTER(c_i64)]),
    "ultr_gsf_saved_bytes": (c_i64, [ctypes.POINTER(GsfDesc), c_i64]),
    "ultr_gsf_score_bytes": (c_i64, [ctypes.POINTER(GsfDesc), c_i64]),
    "ultr_gsf_workspace_bytes": (c_i64, [ctypes.POINTER(GsfDesc), c_i32, c_i32]),
    "ultr_gsf_shuffle": (c_i32, [ctypes.c_uint64, ctypes.c_uint64, c_i32, c_i32, c_vp, c_vp]),
    "ultr_gsf_forward": (c_i32, [ctypes.POINTER(GsfDesc), c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_gsf_backward": (c_i32, [ctypes.POINTER(GsfDesc), c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp,
                                  c_vp, c_vp]),
    "ultr_apply_update": (c_i32, [ctypes.POINTER(UpdateDesc), ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp]),
    "ultr_opt_state_floats": (c_i64, [ctypes.POINTER(UpdateDesc)]),
    "ultr_train_step": (c_i32, [ctypes.POINTER(StepArgs), c_vp]),
    "ultr_click_batch": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_i32, c_vp, c_i32, c_i32, ctypes.c_uint64, ctypes.c_uint64,
                                 c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_click_batch_args": (c_i32, [c_vp, c_vp]),
    "ultr_feed_train_step": (c_i32, [c_vp, c_vp, c_vp]),
    "ultr_online_pick_args": (c_i32, [c_vp, c_vp]),
    "ultr_online_rerank_args": (c_i32, [c_vp, c_vp]),
    "ultr_dbgd_noise_args": (c_i32, [c_vp, c_vp]),
    "ultr_dbgd_interleave_args": (c_i32, [c_vp, c_vp]),
    "ultr_dbgd_grad_args": (c_i32, [c_vp, c_vp]),
    "ultr_nsgd_workspace_bytes": (c_i64, [ctypes.POINTER(DnnDesc), c_i32]),
    "ultr_nsgd_noise_args": (c_i32, [c_vp, c_vp]),
    "ultr_nsgd_memory_args": (c_i32, [c_vp, c_vp]),
    "ultr_propensity_count": (c_i32, [c_vp, c_vp]),
    "ultr_history_pw": (c_i32, [c_vp, c_vp]),
    "ultr_comm_create": (c_i32, [c_i32, c_i32, c_i64, ctypes.POINTER(c_vp)]),
    "ultr_comm_export": (c_i32, [c_vp, c_vp]),
    "ultr_comm_import": (c_i32, [c_vp, c_i32, c_vp]),
    "ultr_comm_allreduce": (c_i32, [c_vp, ctypes.c_uint64, c_vp, c_i64, c_i64, c_vp, c_vp, c_i32, c_vp]),
    "ultr_comm_status": (c_i32, [c_vp, c_vp]),
    "ultr_comm_destroy": (c_i32, [c_vp]),
    "ultr_config_reload": (c_i32, []),
    "ultr_prof_enable": (c_i32, [ctypes.c_uint32, c_i32]),
    "ultr_prof_set_stride": (c_i32, [c_i32]),
    "ultr_prof_collect": (c_i32, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i64)]),
    "ultr_ndcg": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "ultr_ndcg_report": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                 ctypes.c_uint32, c_vp]),
    "ultr_dnn_forward_ndcg": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_i32, c_vp, ctypes.POINTER(c_i32),
                                      c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint32, c_vp]),
    "ultr_metrics_report": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32, ctypes.POINTER(c_i32), c_i32,
                                    ctypes.c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint32, c_vp]),
    "ultr_metrics_long": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(c_i32), c_i32, ctypes.POINTER(c_i32), c_i32,
                                  ctypes.c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint32, c_vp]),
    "ultr_metrics_max_list": (c_i32, []),
    "ultr_dnn_forward_metrics": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_i32, c_vp,
                                         ctypes.POINTER(c_i32), c_i32, ctypes.POINTER(c_i32), c_i32, ctypes.c_float, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_vp, ctypes.c_uint32, c_vp]),
    "ultr_eval_pick": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "ultr_eval_accumulate": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, ctypes.c_uint32, c_vp]),
    "ultr_dnn_eval_set": (c_i32, [ctypes.POINTER(DnnDesc), c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32,
                                  ctypes.POINTER(c_i32), c_i32, ctypes.POINTER(c_i32), c_i32, ctypes.c_float, c_vp, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint32, c_vp]),
}

_LIB = None


def load(path=None):
    """dlopen libultr_hip.so and type every entry point.  Raises if it is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("ULTR_HIP_LIB") or LIB_PATH  # ULTR_HIP_LIB: experiment builds (tools/ab_build.sh)
    if not os.path.exists(p):
        raise RuntimeError(
            "libultr_hip.so not found at %s — build it first: python -c 'import __graft_entry__ as g; g.build()' "
            "(ultra_pytorch_amd has no CPU fallback)" % p)
    try:  # make sure the HIP runtime the process will use is torch's (same SONAME libamdhip64.so.7)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - symbol checks work without torch
        pass
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    got = int(lib.ultr_abi_version())
    if got != ABI_VERSION:
        # a stale or experimental build (ULTR_HIP_LIB) that happens to export every symbol would be called with shifted arguments
        raise RuntimeError("%s reports ABI %d, this binding is written for ABI %d: rebuild the library "
                           "(python -c 'import __graft_entry__ as g; g.build()')" % (p, got, ABI_VERSION))
    if path is None:
        _LIB = lib
    return lib


def make_desc(feature_size, hidden, activation="elu"):
    hidden = list(hidden or [])
    if len(hidden) > ULTR_MAX_HIDDEN:
        raise ValueError("at most %d hidden layers are supported" % ULTR_MAX_HIDDEN)
    if activation not in ACT:
        raise ValueError("activation_func must be one of %s (got %r)" % (sorted(ACT), activation))
    d = DnnDesc()
    d.feature_size = int(feature_size)
    d.n_hidden = len(hidden)
    for i, h in enumerate(hidden):
        d.hidden[i] = int(h)
    d.activation = ACT[activation]
    return d


class UltrHipError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        kind = {-1: "bad argument", -2: "unsupported shape", -3: "workspace too small", -4: "peer wait timed out"}.get(rc, "hipError_t %d" % rc)
        raise UltrHipError("%s failed: %s" % (what, kind))
