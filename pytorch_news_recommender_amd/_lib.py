"""ctypes binding of libnrms_hip.so (the C ABI in include/nrms_hip.h).

There is NO fallback: if the library is missing or a call fails this raises.  The
product path never computes on the CPU and never imports ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NRMS_HIP_LIB") or os.path.join(PKG, "libnrms_hip.so")   # override: diagnostic builds only

NRMS_OK, NRMS_EINVAL, NRMS_ELAUNCH, NRMS_EWORKSPACE = 0, -1, -2, -3     # return codes (include/nrms_hip.h)
NRMS_FLAG_PAD_ROW_ZERO = 1
NRMS_FLAG_DEFER_WQKV = 2
NRMS_FLAG_FWD_SCRATCH_KEPT = 4
NRMS_FLAG_FUSED_SEQ64 = 8
NRMS_FLAG_DEFER_USER_JOIN = 16
NRMS_FLAG_TABLE_ADAM = 32
NRMS_PRECISION_FP32 = 0
NRMS_PRECISION_BF16X3 = 1
NRMS_PRECISION_BF16 = 2
NRMS_PRECISION_FP16 = 3
NRMS_DROPOUT_FIELDS16 = 0x100
NRMS_DROPOUT_SITE_NEWSVEC = 4
NRMS_FP16_KP, NRMS_FP16_DP, NRMS_FP16_QP = 320, 320, 224     # fixed activation pitches of the fp16 mode (include/nrms_hip.h)
PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16": 2, "fp16": 3}


class NrmsError(RuntimeError):
    pass


class EncoderDesc(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("seq_len", C.c_int32), ("d_model", C.c_int32),
                ("n_heads", C.c_int32), ("q_dim", C.c_int32), ("vocab", C.c_int32),
                ("p_drop_embed", C.c_float), ("p_drop_ctx", C.c_float), ("precision", C.c_int32),
                ("use_output_proj", C.c_int32), ("mask_mode", C.c_int32), ("flags", C.c_int32),
                ("seed", C.c_uint64), ("loss_scale", C.c_float), ("p_drop_attn", C.c_float), ("seq_index", C.c_void_p)]


class EncoderWeights(C.Structure):
    _fields_ = [("table", C.c_void_p), ("w_qkv", C.c_void_p), ("b_qkv", C.c_void_p), ("w_o", C.c_void_p),
                ("b_o", C.c_void_p), ("w_add", C.c_void_p), ("b_add", C.c_void_p), ("q_vec", C.c_void_p)]


class EncoderGrads(C.Structure):
    _fields_ = [("table", C.c_void_p), ("w_qkv", C.c_void_p), ("b_qkv", C.c_void_p), ("w_o", C.c_void_p),
                ("b_o", C.c_void_p), ("w_add", C.c_void_p), ("b_add", C.c_void_p), ("q_vec", C.c_void_p)]


class TableAdam(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("step", C.c_int32), ("grad_scale", C.c_float), ("n_nonfinite", C.c_void_p)]


class EncoderActs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("qkv", C.c_void_p), ("attn", C.c_void_p), ("ctx", C.c_void_p),
                ("t", C.c_void_p), ("w", C.c_void_p), ("scratch", C.c_void_p)]


class SegPoolDesc(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_seg", C.c_int64), ("nnz", C.c_int64), ("d", C.c_int32), ("q", C.c_int32),
                ("precision", C.c_int32), ("flags", C.c_int32)]


NRMS_SEGPOOL_ROWS_UNIQUE = 1


class ClickGraphDesc(C.Structure):
    _fields_ = [("n_users", C.c_int64), ("n_news", C.c_int64), ("n_edges", C.c_int64), ("user_ptr", C.c_void_p),
                ("user_news", C.c_void_p), ("news_ptr", C.c_void_p), ("news_users", C.c_void_p)]


class NewsFeatures(C.Structure):
    _fields_ = [("n", C.c_int64), ("d_text", C.c_int32), ("d_cat", C.c_int32), ("n_cat", C.c_int32), ("n_sub", C.c_int32),
                ("p_drop", C.c_float), ("seed", C.c_uint64), ("title_vec", C.c_void_p), ("abst_vec", C.c_void_p),
                ("cat_table", C.c_void_p), ("sub_table", C.c_void_p), ("categ", C.c_void_p), ("subcateg", C.c_void_p)]


class NewsvecDesc(C.Structure):
    _fields_ = [("n_slots", C.c_int64), ("n_rows", C.c_int32), ("d", C.c_int32), ("precision", C.c_int32),
                ("p_drop", C.c_float), ("seed", C.c_uint64)]


# name -> (restype, argtypes).  Every symbol include/nrms_hip.h declares.
SIGNATURES = {
    "nrms_encoder_fwd": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(EncoderActs), C.c_void_p, C.c_void_p]),
    "nrms_encoder_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "nrms_encoder_fwd_scratch_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "nrms_encoder_fused_qkv_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "nrms_encoder_bwd": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(EncoderActs), C.c_void_p, C.POINTER(EncoderGrads), C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_encoder_bwd_adam": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(EncoderActs), C.c_void_p, C.POINTER(EncoderGrads), C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.POINTER(TableAdam), C.c_void_p]),
    "nrms_encoder_bwd_wqkv": (C.c_int, [C.POINTER(EncoderDesc), C.c_void_p, C.c_void_p, C.POINTER(EncoderActs),
                                        C.POINTER(EncoderGrads), C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_encoder_join": (C.c_int, [C.c_void_p]),
    "nrms_sanitize_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "nrms_sanitize_ids_i32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "nrms_title_dedup": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "nrms_click_score_indexed": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_click_score_fwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "nrms_click_score_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_ce_loss_fwd_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                       C.c_void_p]),
    "nrms_adam_step": (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                 C.c_double, C.c_double, C.c_double, C.c_int32, C.c_float, C.c_void_p]),
    "nrms_adam_step_guarded": (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_double, C.c_double, C.c_double, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "nrms_adam_step_rest": (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_double, C.c_double, C.c_double, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "nrms_grad_guard": (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_segment_pool_workspace_bytes": (C.c_size_t, [C.POINTER(SegPoolDesc)]),
    "nrms_segment_pool_fwd": (C.c_int, [C.POINTER(SegPoolDesc)] + [C.c_void_p] * 10 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_segment_pool_bwd": (C.c_int, [C.POINTER(SegPoolDesc)] + [C.c_void_p] * 12 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_hier_tree_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "nrms_hier_tree_build": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 16 + [C.c_size_t, C.c_void_p]),
    "nrms_hier_add_embedding_fwd": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_sequence_partition_count_ints": (C.c_size_t, [C.c_int32]),
    "nrms_sequence_partition": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_encoder_empty_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "nrms_encoder_empty_saved_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "nrms_encoder_empty_fwd": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "nrms_encoder_empty_bwd": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EncoderGrads),
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_csr_from_padded": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_graph_sample_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "nrms_graph_sample_neighbors": (C.c_int, [C.POINTER(ClickGraphDesc), C.c_int64, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_graph_resolve_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "nrms_graph_resolve_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
                                + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_negative_sample_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "nrms_negative_sample": (C.c_int, [C.c_int64] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_uint64] + [C.c_void_p] * 3
                             + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_catalogue_negative_sample_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "nrms_catalogue_negative_sample": (C.c_int, [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                                 C.c_uint64] + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_hier_add_embedding_bwd_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "nrms_hier_add_embedding_bwd": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]),
    "nrms_hier_match": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 11 + [C.c_void_p]),
    "nrms_hier_score_fwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "nrms_hier_score_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9 + [C.c_float, C.c_float] + [C.c_void_p] * 5 + [C.c_void_p]),
    "nrms_impression_auc": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "nrms_impression_metrics": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
                                + [C.c_void_p] * 5 + [C.c_void_p]),
    "nrms_topk_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_topk_grouped_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_topk_grouped_dot": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
                              + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_sections_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_topk_sections_dot": (C.c_int, [C.c_int32, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 6 + [C.c_int32]
                               + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
                      + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_biased_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_biased": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
                             + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_biased_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot_biased": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
                             + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_windowed_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_windowed": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                               + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_after_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_after": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32]
                            + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_deep_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_deep": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                           + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_windowed_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot_windowed": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32]
                               + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_tagged_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_tagged": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
                             + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_capped_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_capped": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
                             + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_adjusted_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_adjusted": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
                               + [C.c_void_p] + [C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_adjusted_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot_adjusted": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
                               + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_request_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_request": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                              + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3
                              + [C.c_size_t, C.c_void_p]),
    "nrms_topk_dot_request_capped_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "nrms_topk_dot_request_capped": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                                     + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3
                                     + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_request_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot_request": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                              + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 3
                              + [C.c_size_t, C.c_void_p]),
    "nrms_rank_dot_tagged_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_rank_dot_tagged": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
                             + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_catalogue_f16_pitch": (C.c_int32, [C.c_int32]),
    "nrms_catalogue_pack_f16": (C.c_int, [C.c_int64, C.c_int32] + [C.c_void_p] * 4),
    "nrms_topk_dot_coarse_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_topk_dot_coarse": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
                             + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    "nrms_softmax_sample_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_softmax_sample_dot": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_float, C.c_uint64, C.c_void_p,
                                          C.c_int32] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "nrms_mmr_rerank_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "nrms_mmr_rerank": (C.c_int, [C.c_int32] * 4 + [C.c_int64, C.c_float] + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]),
    "nrms_attribution_dot_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "nrms_attribution_dot": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 11
                             + [C.c_size_t, C.c_void_p]),
    "nrms_softmax_sample_noise": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_logsumexp_dot_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "nrms_logsumexp_dot": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                           + [C.c_void_p] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_logsumexp_dot_mass": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
                                + [C.c_void_p] + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_hier_query":(C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 10 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "nrms_dropout_keep_mask": (C.c_int, [C.c_uint64, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_void_p,
                                         C.c_void_p]),
    "nrms_layernorm_fwd": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "nrms_layernorm_bwd_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "nrms_layernorm_bwd": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_news_features_fwd": (C.c_int, [C.POINTER(NewsFeatures), C.c_void_p, C.c_void_p]),
    "nrms_news_features_bwd": (C.c_int, [C.POINTER(NewsFeatures), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "nrms_newsvec_saved_bytes": (C.c_size_t, [C.POINTER(NewsvecDesc)]),
    "nrms_newsvec_workspace_bytes": (C.c_size_t, [C.POINTER(NewsvecDesc)]),
    "nrms_newsvec_fwd": (C.c_int, [C.POINTER(NewsvecDesc)] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                                C.c_void_p]),
    "nrms_newsvec_bwd": (C.c_int, [C.POINTER(NewsvecDesc)] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 4
                         + [C.c_size_t, C.c_void_p]),
    "nrms_newsvec_distinct": (C.c_int, [C.POINTER(NewsvecDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrms_newsvec_rows_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "nrms_newsvec_rows_fwd": (C.c_int, [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "nrms_pooled_ce_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "nrms_pooled_ce_fwd_bwd": (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 4
                               + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nrms_timing_enable": (None, [C.c_int]),
    "nrms_timing_reset": (None, []),
    "nrms_timing_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "nrms_last_error": (C.c_char_p, []),
    "nrms_version": (C.c_char_p, []),
}

_lib = None


def load():
    """Load the library (once) and bind every declared symbol.  Raises NrmsError if the
    shared object is absent -- build it with ``python -m pytorch_news_recommender_amd.build``."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NrmsError(
            "libnrms_hip.so not found at %s: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m pytorch_news_recommender_amd.build`." % LIB_PATH)
    # torch ships its own libamdhip64; it must be resident first so this library binds to the
    # SAME HIP runtime instance (streams / device pointers are shared with torch).  Loading
    # libnrms_hip.so before torch would pull in /opt/rocm's copy and split the process in two.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the header and the .so disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().nrms_last_error()
        raise NrmsError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())
