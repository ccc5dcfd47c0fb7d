"""ctypes binding of libbtsbot_hip.so (include/btsbot_hip.h).

There is no CPU fallback: if the shared library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (BTSBOT_AMD_LIB: another build of the same library, for A/B timing of kernel variants -- tools/build_variant.sh)
LIB_PATH = os.environ.get("BTSBOT_AMD_LIB") or os.path.join(_HERE, "libbtsbot_hip.so")
ABI_VERSION = 1

OK = 0
ERR_INVALID_ARG = -1
ERR_STATE = -5
WIRING = {"mm_ConvNeXt": 0, "ConvNeXt": 1, "frozen_fusion": 2, "um_nn": 3, "mm_MaxViT": 4,
          "MaxViT": 5, "frozen_fusion_MaxViT": 6}
PRECISION = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "f16": 2, "fp16": 2,
             "float16": 2, "fp8": 3, "f16x2": 4}

# every symbol include/btsbot_hip.h declares (tests/test_abi.py checks the export list)
SYMBOLS = [
    "btsbot_last_error", "btsbot_abi_version", "btsbot_create", "btsbot_destroy",
    "btsbot_param_count", "btsbot_param_floats", "btsbot_param_info_at", "btsbot_pack_params",
    "btsbot_pack_params_train",
    "btsbot_workspace_bytes", "btsbot_reserve", "btsbot_forward", "btsbot_set_debug",
    "btsbot_read_tap", "btsbot_bce_fwd_bwd", "btsbot_adamw_step",
    "btsbot_set_profile", "btsbot_profile_categories", "btsbot_profile_category_name",
    "btsbot_profile_collect",
    "btsbot_op_gemm", "btsbot_op_dwconv_ln", "btsbot_op_stem", "btsbot_op_ln_patch", "btsbot_op_wgrad",
    "btsbot_op_gemm_gated", "btsbot_op_gemm_resid_ln",
    "btsbot_op_mv_attn", "btsbot_op_mv_attn_block", "btsbot_op_mv_part", "btsbot_op_mv_dw3", "btsbot_op_mv_dw3_groups",
    "btsbot_op_mv_mbconv_front", "btsbot_op_mv_mbconv_front_tiles", "btsbot_op_mv_se", "btsbot_op_mv_stem",
    "btsbot_op_mvt_bn_row_blocks", "btsbot_op_mvt_dw3_bwd_w_row_blocks", "btsbot_op_mvt_attn_bwd_groups_per_head",
    "btsbot_op_mvt_bn_fwd", "btsbot_op_mvt_bn_bwd", "btsbot_op_mvt_dw3_fwd", "btsbot_op_mvt_dw3_bwd_in",
    "btsbot_op_mvt_dw3_bwd_w", "btsbot_op_mvt_attn_bwd", "btsbot_op_mvt_se_fwd", "btsbot_op_mvt_se_bwd",
    "btsbot_op_mvt_avgpool2_bwd", "btsbot_op_mvt_col2im3", "btsbot_op_mvt_unpack_conv3_grad", "btsbot_op_mvt_gelu_fwd",
    "btsbot_op_mvt_gelu_bwd", "btsbot_op_mvt_bcast_set",
    "btsbot_op_cnt_dwln_bwd_rows", "btsbot_op_cnt_dw3ln_bwd_rows", "btsbot_op_cnt_dwln_bwd", "btsbot_op_cnt_dw3ln_bwd",
    "btsbot_op_cnt_ln_bwd", "btsbot_op_cnt_ln_dw1_bwd", "btsbot_op_cnt_dw_plain", "btsbot_op_cnt_dw_wgrad",
    "btsbot_op_cnt_colsum_f32", "btsbot_op_cnt_stem_dgrad",
    "btsbot_op_cnt_mlp_bwd_planes", "btsbot_op_cnt_mlp_bwd_slices", "btsbot_op_cnt_s2mlp_bwd_rows", "btsbot_op_cnt_mlp_bwd",
    "btsbot_op_cnt_s2mlp_bwd", "btsbot_op_cnt_fused_mlp", "btsbot_op_cnt_fc2_grads",
    "btsbot_op_head16_supported", "btsbot_op_head",
    "btsbot_op_cn_stage3_supported", "btsbot_op_cn_stage3_hfrag_bytes", "btsbot_op_cn_stage3", "btsbot_op_cn_pack_s3",
    "btsbot_op_cn_fp8_scale",
    "btsbot_op_cn_stage2_supported", "btsbot_op_cn_stage2_alerts", "btsbot_op_cn_stage2", "btsbot_op_cn_stage2_rows",
    "btsbot_op_cn_pack_s2p",
    "btsbot_op_ht_lin_is_wide", "btsbot_op_ht_lin_fwd", "btsbot_op_ht_act_bwd", "btsbot_op_ht_lin_bwd_in",
    "btsbot_op_ht_lin_bwd_w_kind", "btsbot_op_ht_lin_bwd_w", "btsbot_op_ht_bn_fwd", "btsbot_op_ht_bn_bwd",
    "btsbot_op_ht_feat_rows", "btsbot_op_ht_logits", "btsbot_op_ht_copy_cols",
    "btsbot_op_ht_bn_eval_fwd", "btsbot_op_ht_bn_bwd_in",
    "btsbot_reserve_train", "btsbot_forward_train", "btsbot_backward", "btsbot_debug_stamps",
    "btsbot_forward_keep_eval", "btsbot_backward_inputs",
    "btsbot_grad_buckets", "btsbot_wait_grad_bucket", "btsbot_allreduce_grads", "btsbot_use_workspace", "btsbot_set_option",
    "btsbot_augment", "btsbot_eval_metrics", "btsbot_prep_triplets", "btsbot_alert_features",
    "btsbot_split_labels", "btsbot_decode_stamps_workspace", "btsbot_decode_stamps",
    "btsbot_policy_eval", "btsbot_alert_histograms", "btsbot_trigger_reset", "btsbot_trigger_update", "btsbot_trigger_load",
    "btsbot_trigger_rehash", "btsbot_feature_reset", "btsbot_feature_update", "btsbot_feature_load", "btsbot_feature_rehash",
    "btsbot_embed_width", "btsbot_forward_embed",
    "btsbot_knn_bank_bytes", "btsbot_knn_pack_bank", "btsbot_knn_splits", "btsbot_knn_workspace", "btsbot_knn_query",
    "btsbot_knn_workspace_grouped", "btsbot_knn_query_grouped",
    "btsbot_knn_radius_workspace", "btsbot_knn_radius_count", "btsbot_knn_radius_fill",
    "btsbot_knn_rank_workspace", "btsbot_knn_rank_count", "btsbot_knn_rank_fill",
    "btsbot_graph_components", "btsbot_dbscan_labels",
    "btsbot_grid_finite", "btsbot_grid_cells", "btsbot_grid_radius_count", "btsbot_grid_radius_fill", "btsbot_grid_knn",
    "btsbot_layout_smooth_knn", "btsbot_layout_symmetrize_workspace", "btsbot_layout_symmetrize", "btsbot_layout_init",
    "btsbot_layout_epochs", "btsbot_layout_smooth_knn_query", "btsbot_layout_transform",
    "btsbot_lof_fit", "btsbot_lof_score",
    "btsbot_knn_graph_merge", "btsbot_knn_graph_compact",
    "btsbot_kmeans_workspace", "btsbot_kmeans_update", "btsbot_ivf_list_rows", "btsbot_ivf_layout", "btsbot_ivf_workspace",
    "btsbot_ivf_query", "btsbot_ivf_layout_groups", "btsbot_ivf_workspace_grouped", "btsbot_ivf_query_grouped",
    "btsbot_mst_offer_knn", "btsbot_mst_offer_csr", "btsbot_mst_merge", "btsbot_hdbscan_tree",
    "btsbot_hdbscan_model", "btsbot_cluster_offer_knn", "btsbot_cluster_offer_csr", "btsbot_cluster_assign",
]
LOF_MAX_K = 64                               # csrc/lof.hip
MST_MAX_K = 64                               # csrc/mr_offer.hip: search_k
HDBSCAN_METHOD = {"eom": 0, "leaf": 1}       # enum btsbot_hdbscan_method
LAYOUT_MAX_K, LAYOUT_MAX_NEGATIVES = 64, 64
KNN_METRIC = {"euclidean": 0, "cosine": 1}   # enum btsbot_knn_metric
KNN_MAX_DIM, KNN_MAX_K, KNN_MAX_SPLITS = 1024, 64, 32
KNN_EXCLUDE_SAME, KNN_ONE_PER_GROUP = 1, 2   # enum btsbot_knn_flags
KNN_MAX_K_ONE_PER_GROUP = 32                 # k's cap under KNN_ONE_PER_GROUP
KNN_GRAPH_DISTINCT = 1                       # enum btsbot_knn_graph_flags (csrc/knn_graph.hip)
IVF_MAX_LISTS, IVF_MAX_NPROBE = 65536, 32    # csrc/ivf.hip (nprobe's cap is the merge's KNN_MAX_SPLITS)
KMEANS_CHUNK = 64                            # csrc/ivf.hip: rows per partial sum of btsbot_kmeans_update
GRID_MAX_CELLS, GRID_MAX_K = 4096, 64         # csrc/grid.hip
GRID_LANES = (0, 1, 4, 8, 16, 32, 64)        # lanes per query row of btsbot_grid_radius_* (0: the library's choice)
EMBEDDING = {"features": 0, "hidden": 1}   # enum btsbot_embedding
# enum btsbot_stamp_status: what btsbot_decode_stamps says of each stamp
STAMP_STATUS = {"OK": 0, "BAD_GZIP": 1, "BAD_DEFLATE": 2, "TOO_LARGE": 3, "BAD_TRAILER": 4, "BAD_FITS": 5,
                "UNSUPPORTED": 6}
STAMP_CAP = 28800   # BTSBOT_STAMP_CAP


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("wiring", C.c_int32), ("precision", C.c_int32),
        ("depths", C.c_int32 * 4), ("dims", C.c_int32 * 4), ("image_size", C.c_int32),
        ("head_norm", C.c_int32), ("n_meta", C.c_int32),
        ("meta_fc1", C.c_int32), ("meta_fc2", C.c_int32),
        ("comb_fc1", C.c_int32), ("comb_fc2", C.c_int32),
        ("meta_dropout", C.c_float), ("comb_dropout", C.c_float),
    ]


class ParamInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char * 96), ("offset", C.c_int64), ("numel", C.c_int64),
        ("ndim", C.c_int32), ("shape", C.c_int32 * 4), ("is_buffer", C.c_int32),
    ]


TRIGGER_COUNTER_ROWS = 16   # BTSBOT_TRIGGER_COUNTER_ROWS


class TriggerTable(C.Structure):   # struct btsbot_trigger_table
    _fields_ = [
        ("key", C.c_void_p), ("n_alerts", C.c_void_p), ("min_magpsf", C.c_void_p), ("last_jd", C.c_void_p),
        ("count", C.c_void_p), ("trigger", C.c_void_p), ("counters", C.c_void_p),
        ("capacity", C.c_int32), ("n_policies", C.c_int32),
    ]


class FeatureTable(C.Structure):   # struct btsbot_feature_table
    _fields_ = [
        ("key", C.c_void_p), ("n_alerts", C.c_void_p), ("first_jd", C.c_void_p), ("last_jd", C.c_void_p),
        ("peak_mag", C.c_void_p), ("peak_jd", C.c_void_p), ("max_mag", C.c_void_p), ("counters", C.c_void_p),
        ("capacity", C.c_int32),
    ]


class BtsbotHipError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load the shared library once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise BtsbotHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C btsbot_amd/csrc`.  btsbot_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    L.btsbot_last_error.restype = C.c_char_p
    L.btsbot_last_error.argtypes = []
    L.btsbot_abi_version.restype = i32
    L.btsbot_abi_version.argtypes = []
    L.btsbot_create.restype = i32
    L.btsbot_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.btsbot_destroy.restype = i32
    L.btsbot_destroy.argtypes = [vp]
    L.btsbot_param_count.restype = i32
    L.btsbot_param_count.argtypes = [vp]
    L.btsbot_param_floats.restype = i64
    L.btsbot_param_floats.argtypes = [vp]
    L.btsbot_param_info_at.restype = i32
    L.btsbot_param_info_at.argtypes = [vp, i32, C.POINTER(ParamInfo)]
    L.btsbot_pack_params.restype = i32
    L.btsbot_pack_params.argtypes = [vp, vp, vp]
    L.btsbot_pack_params_train.restype = i32
    L.btsbot_pack_params_train.argtypes = [vp, vp, vp]
    L.btsbot_workspace_bytes.restype = i64
    L.btsbot_workspace_bytes.argtypes = [vp, i32]
    L.btsbot_reserve.restype = i32
    L.btsbot_reserve.argtypes = [vp, i32]
    L.btsbot_forward.restype = i32
    L.btsbot_forward.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_uint64, vp]
    L.btsbot_embed_width.restype = i32
    L.btsbot_embed_width.argtypes = [vp, i32]
    L.btsbot_forward_embed.restype = i32
    L.btsbot_forward_embed.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.btsbot_set_debug.restype = i32
    L.btsbot_set_debug.argtypes = [vp, i32]
    L.btsbot_read_tap.restype = i64
    L.btsbot_read_tap.argtypes = [vp, C.c_char_p, vp, i64, vp]
    L.btsbot_set_profile.restype = i32
    L.btsbot_set_profile.argtypes = [vp, i32]
    L.btsbot_profile_categories.restype = i32
    L.btsbot_profile_categories.argtypes = []
    L.btsbot_profile_category_name.restype = C.c_char_p
    L.btsbot_profile_category_name.argtypes = [i32]
    L.btsbot_profile_collect.restype = i32
    L.btsbot_profile_collect.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i64)]
    L.btsbot_op_gemm.restype = i32
    L.btsbot_op_gemm.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.btsbot_op_wgrad.restype = i32
    L.btsbot_op_wgrad.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp]
    L.btsbot_op_gemm_gated.restype = i32
    L.btsbot_op_gemm_gated.argtypes = [i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp]
    L.btsbot_op_gemm_resid_ln.restype = i32
    L.btsbot_op_gemm_resid_ln.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.btsbot_op_dwconv_ln.restype = i32
    L.btsbot_op_dwconv_ln.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.btsbot_op_stem.restype = i32
    L.btsbot_op_stem.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.btsbot_op_ln_patch.restype = i32
    L.btsbot_op_ln_patch.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp]
    L.btsbot_op_mv_attn.restype = i32
    L.btsbot_op_mv_attn.argtypes = [i32, i32, vp, vp, vp, i32, i32, i32, i32, vp]
    L.btsbot_op_mv_attn_block.restype = i32
    L.btsbot_op_mv_attn_block.argtypes = [i32] + [vp] * 10 + [i32, i32, i32, vp]
    L.btsbot_op_mv_part.restype = i32
    L.btsbot_op_mv_part.argtypes = [i32] + [vp] * 17 + [i32, i32, i32, i32, vp]
    L.btsbot_op_mv_dw3.restype = i32
    L.btsbot_op_mv_dw3.argtypes = [i32, i32] + [vp] * 6 + [i32, i32, i32, i32, vp]
    L.btsbot_op_mv_dw3_groups.restype = i32
    L.btsbot_op_mv_dw3_groups.argtypes = [i32, i32, i32]
    L.btsbot_op_mv_mbconv_front.restype = i32
    L.btsbot_op_mv_mbconv_front.argtypes = [i32] + [vp] * 8 + [i32, i32, i32, i32, i32, vp]
    L.btsbot_op_mv_mbconv_front_tiles.restype = i32
    L.btsbot_op_mv_mbconv_front_tiles.argtypes = [i32, i32]
    L.btsbot_op_mv_se.restype = i32
    L.btsbot_op_mv_se.argtypes = [i32] + [vp] * 6 + [i32, i32, i32, i32, f32, vp]
    L.btsbot_op_mv_stem.restype = i32
    L.btsbot_op_mv_stem.argtypes = [i32] + [vp] * 6 + [i32] + [vp] * 3 + [i32, vp]
    for name, args in (("bn_row_blocks", [i64]), ("dw3_bwd_w_row_blocks", [i64]), ("attn_bwd_groups_per_head", [i64, i32]),
                       ("bn_fwd", [vp] * 7 + [i64, i32, i32, vp]), ("bn_bwd", [vp] * 8 + [i64, i32, i32, i32, vp]),
                       ("dw3_fwd", [vp] * 4 + [i32] * 4 + [vp]), ("dw3_bwd_in", [vp] * 3 + [i32] * 4 + [vp]),
                       ("dw3_bwd_w", [vp] * 4 + [i32] * 4 + [vp]), ("attn_bwd", [vp] * 5 + [i32] * 4 + [vp]),
                       ("se_fwd", [vp] * 10 + [i32] * 4 + [vp]), ("se_bwd", [vp] * 13 + [i32] * 4 + [vp]),
                       ("avgpool2_bwd", [vp, vp] + [i32] * 4 + [vp]), ("col2im3", [vp, vp] + [i32] * 3 + [vp]),
                       ("unpack_conv3_grad", [vp, vp] + [i32] * 3 + [vp]), ("gelu_fwd", [vp, vp, i64, vp]),
                       ("gelu_bwd", [vp, vp, i64, vp]), ("bcast_set", [vp, vp, i32, i32, i32, f32, vp])):
        fn = getattr(L, "btsbot_op_mvt_" + name)
        fn.restype = i32
        fn.argtypes = args
    for name, args in (("dwln_bwd_rows", [i32] * 3), ("dw3ln_bwd_rows", [i32]),
                       ("dwln_bwd", [vp] * 7 + [i32, vp] + [i32] * 4 + [i64, vp]),
                       ("dw3ln_bwd", [vp] * 7 + [i32, vp] + [i32] * 4 + [i64, vp]),
                       ("ln_bwd", [vp] * 6 + [i64, i32, vp, i32, i32, vp]),
                       ("ln_dw1_bwd", [vp] * 7 + [i32] + [vp] * 4 + [i64, i32, vp]),
                       ("dw_plain", [vp, vp, i32, vp, vp, vp, vp] + [i32] * 4 + [vp]),
                       ("dw_wgrad", [vp] * 4 + [i32] * 3 + [vp]), ("colsum_f32", [vp, vp, i32, i32, vp]),
                       ("stem_dgrad", [vp, vp, vp, i32, i32, vp]),
                       ("mlp_bwd_planes", [i32]), ("mlp_bwd_slices", [i32, i32]), ("s2mlp_bwd_rows", []),
                       ("mlp_bwd", [i32, i32] + [vp] * 10 + [i32, i32, vp]), ("s2mlp_bwd", [i32, i32] + [vp] * 6 + [i32, vp]),
                       ("fused_mlp", [i32, i32] + [vp] * 8 + [i32, vp]), ("fc2_grads", [vp] * 8 + [i32, i32, vp])):
        fn = getattr(L, "btsbot_op_cnt_" + name)
        fn.restype = i32
        fn.argtypes = args
    L.btsbot_op_head16_supported.restype = i32
    L.btsbot_op_head16_supported.argtypes = [i32] * 6 + [C.POINTER(i32)]
    L.btsbot_op_head.restype = i32
    L.btsbot_op_head.argtypes = ([i32, vp, i32, vp, vp, vp, i32] + [vp] * 6 + [i32, vp, vp, i32, i32, i32, C.POINTER(i32),
                                 C.POINTER(vp), C.POINTER(vp), i32] + [vp] * 4 + [i32, vp])
    L.btsbot_op_cn_stage3_supported.restype = i32
    L.btsbot_op_cn_stage3_supported.argtypes = [i32] * 3
    L.btsbot_op_cn_stage3_hfrag_bytes.restype = i64
    L.btsbot_op_cn_stage3_hfrag_bytes.argtypes = [i32] * 3
    L.btsbot_op_cn_stage3.restype = i32
    L.btsbot_op_cn_stage3.argtypes = [i32] * 4 + [vp, i32] + [C.POINTER(vp)] * 9 + [vp]
    L.btsbot_op_cn_pack_s3.restype = i32
    L.btsbot_op_cn_pack_s3.argtypes = [i32, vp, vp, i32, i32, i32, vp, vp, vp]
    L.btsbot_op_cn_stage2_supported.restype = i32
    L.btsbot_op_cn_stage2_supported.argtypes = [i32] * 3
    L.btsbot_op_cn_stage2_alerts.restype = i32
    L.btsbot_op_cn_stage2_alerts.argtypes = [i32] * 2
    L.btsbot_op_cn_stage2.restype = i32
    L.btsbot_op_cn_stage2.argtypes = [i32] * 4 + [vp, i32] + [C.POINTER(vp)] * 9 + [vp] * 6 + [C.POINTER(vp)] * 4 + [vp, vp]
    L.btsbot_op_cn_stage2_rows.restype = i32
    L.btsbot_op_cn_stage2_rows.argtypes = [i32, vp, i64] + [vp] * 8
    L.btsbot_op_cn_pack_s2p.restype = i32
    L.btsbot_op_cn_pack_s2p.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.btsbot_op_cn_fp8_scale.restype = i32
    L.btsbot_op_cn_fp8_scale.argtypes = [vp, vp, i64, i32, vp, vp]
    for name, args in (("lin_is_wide", [i32] * 4),
                       ("lin_fwd", [vp, i32, vp, vp, vp, vp] + [i32] * 5 + [vp, f32, vp]),
                       ("act_bwd", [vp, i32, vp, vp, i32, i32, i32, vp, f32, vp]),
                       ("lin_bwd_in", [vp, vp, vp] + [i32] * 4 + [vp]), ("lin_bwd_w_kind", [vp, i32, vp, i32, i32]),
                       ("lin_bwd_w", [vp, vp, i32, vp, vp, i32, i32, i32, vp]),
                       ("bn_fwd", [vp, i32, i32] + [vp] * 8), ("bn_bwd", [vp, i32, i32] + [vp] * 6),
                       ("bn_eval_fwd", [vp, i32, i32] + [vp] * 8), ("bn_bwd_in", [vp, i32, i32] + [vp] * 6 + [i32, vp]),
                       ("feat_rows", [vp, i32, vp, vp, vp, i32, i32, vp]), ("logits", [vp, vp, vp, i32, vp]),
                       ("copy_cols", [vp, i32, vp, i32, i32, i32, vp])):
        fn = getattr(L, "btsbot_op_ht_" + name)
        fn.restype = i32
        fn.argtypes = args
    L.btsbot_debug_stamps.restype = i32
    L.btsbot_debug_stamps.argtypes = [vp, vp]
    L.btsbot_reserve_train.restype = i32
    L.btsbot_reserve_train.argtypes = [vp, i32, i32]
    L.btsbot_forward_train.restype = i32
    L.btsbot_forward_train.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]
    L.btsbot_backward.restype = i32
    L.btsbot_backward.argtypes = [vp, vp, vp, i32, i32, vp]
    L.btsbot_forward_keep_eval.restype = i32
    L.btsbot_forward_keep_eval.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.btsbot_backward_inputs.restype = i32
    L.btsbot_backward_inputs.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.btsbot_grad_buckets.restype = i32
    L.btsbot_grad_buckets.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64)]
    L.btsbot_wait_grad_bucket.restype = i32
    L.btsbot_wait_grad_bucket.argtypes = [vp, i32, vp]
    L.btsbot_set_option.restype = i32
    L.btsbot_set_option.argtypes = [vp, C.c_char_p, i32]
    L.btsbot_use_workspace.restype = i32
    L.btsbot_use_workspace.argtypes = [vp, i32, vp, i64]
    L.btsbot_allreduce_grads.restype = i32
    L.btsbot_allreduce_grads.argtypes = [vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), vp]
    L.btsbot_bce_fwd_bwd.restype = i32
    L.btsbot_bce_fwd_bwd.argtypes = [vp, vp, f32, i32, i32, vp, vp, vp]
    L.btsbot_adamw_step.restype = i32
    L.btsbot_adamw_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, vp]
    L.btsbot_augment.restype = i32
    L.btsbot_augment.argtypes = [vp, vp, vp, vp, i32, vp]
    L.btsbot_prep_triplets.restype = i32
    L.btsbot_prep_triplets.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.btsbot_alert_features.restype = i32
    L.btsbot_alert_features.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.btsbot_split_labels.restype = i32
    L.btsbot_split_labels.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.btsbot_decode_stamps_workspace.restype = i64
    L.btsbot_decode_stamps_workspace.argtypes = [i32]
    L.btsbot_decode_stamps.restype = i32
    L.btsbot_decode_stamps.argtypes = [vp, vp, i32, vp, vp, vp, vp, i64, vp]
    L.btsbot_policy_eval.restype = i32
    L.btsbot_policy_eval.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_double), i32, vp, vp, vp, vp]
    L.btsbot_alert_histograms.restype = i32
    L.btsbot_alert_histograms.argtypes = [vp, vp, vp, i64, C.POINTER(C.c_double), i32, C.POINTER(C.c_double), i32,
                                          C.POINTER(C.c_double), i32, vp, vp]
    L.btsbot_trigger_reset.restype = i32
    L.btsbot_trigger_reset.argtypes = [C.POINTER(TriggerTable), vp]
    L.btsbot_trigger_update.restype = i32
    L.btsbot_trigger_update.argtypes = [C.POINTER(TriggerTable), C.POINTER(C.c_double), vp, vp, i32, i32, vp, vp, vp, vp, vp,
                                        vp, vp]
    L.btsbot_trigger_load.restype = i32
    L.btsbot_trigger_load.argtypes = [C.POINTER(TriggerTable), i32, vp, vp, vp, vp, vp, vp, vp]
    L.btsbot_trigger_rehash.restype = i32
    L.btsbot_trigger_rehash.argtypes = [C.POINTER(TriggerTable), C.POINTER(TriggerTable), C.c_double, vp]
    L.btsbot_feature_reset.restype = i32
    L.btsbot_feature_reset.argtypes = [C.POINTER(FeatureTable), vp]
    L.btsbot_feature_update.restype = i32
    L.btsbot_feature_update.argtypes = [C.POINTER(FeatureTable), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.btsbot_feature_load.restype = i32
    L.btsbot_feature_load.argtypes = [C.POINTER(FeatureTable), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.btsbot_feature_rehash.restype = i32
    L.btsbot_feature_rehash.argtypes = [C.POINTER(FeatureTable), C.POINTER(FeatureTable), C.c_double, vp]
    L.btsbot_knn_bank_bytes.restype = i64
    L.btsbot_knn_bank_bytes.argtypes = [i64, i32]
    L.btsbot_knn_pack_bank.restype = i32
    L.btsbot_knn_pack_bank.argtypes = [vp, i64, i64, i32, i32, vp, i64, vp]
    L.btsbot_knn_splits.restype = i32
    L.btsbot_knn_splits.argtypes = [i64, i64, i32, i32]
    L.btsbot_knn_workspace.restype = i64
    L.btsbot_knn_workspace.argtypes = [i64, i64, i32, i32, i32]
    L.btsbot_knn_query.restype = i32
    L.btsbot_knn_query.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i64, i32, vp, vp, vp, i64, vp]
    L.btsbot_knn_workspace_grouped.restype = i64
    L.btsbot_knn_workspace_grouped.argtypes = [i64, i64, i32, i32, i32, i32]
    L.btsbot_knn_query_grouped.restype = i32
    L.btsbot_knn_query_grouped.argtypes = L.btsbot_knn_query.argtypes + [vp, vp, i32]
    L.btsbot_knn_radius_workspace.restype = i64
    L.btsbot_knn_radius_workspace.argtypes = [i64, i32]
    L.btsbot_knn_radius_count.restype = i32
    L.btsbot_knn_radius_count.argtypes = [vp, i64, vp, i64, i32, i32, vp, i64, i32, vp, vp, i32, vp, vp, i64, vp]
    L.btsbot_knn_radius_fill.restype = i32
    L.btsbot_knn_radius_fill.argtypes = [vp, i64, vp, vp, i64, i32, i32, vp, i64, i32, vp, vp, i32, vp, vp, i64, vp, vp, vp,
                                         vp, vp, i64, vp]
    L.btsbot_knn_rank_workspace.restype = i64
    L.btsbot_knn_rank_workspace.argtypes = [i64, i32, i32]
    rank_head = [vp, i64, vp, vp, i64, i32, i32, vp, i32, i64, i32, vp, vp, i32]
    L.btsbot_knn_rank_count.restype = i32
    L.btsbot_knn_rank_count.argtypes = rank_head + [vp, vp, vp, vp, i64, vp]
    L.btsbot_knn_rank_fill.restype = i32
    L.btsbot_knn_rank_fill.argtypes = rank_head + [vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.btsbot_graph_components.restype = i32
    L.btsbot_graph_components.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    L.btsbot_dbscan_labels.restype = i32
    L.btsbot_dbscan_labels.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp]
    L.btsbot_grid_finite.restype = i32
    L.btsbot_grid_finite.argtypes = [vp, i64, vp, vp]
    L.btsbot_grid_cells.restype = i32
    L.btsbot_grid_cells.argtypes = [vp, i64, vp, i32, vp, vp, vp]
    grid = [vp, i32, vp, vp, vp, vp, i64, i64, vp, i32]   # geom, cells, cell_start, points, rows, groups, n_bank, self, qgroups, flags
    L.btsbot_grid_radius_count.restype = i32
    L.btsbot_grid_radius_count.argtypes = [vp, i64, vp] + grid + [i32, vp, vp, vp]
    L.btsbot_grid_radius_fill.restype = i32
    L.btsbot_grid_radius_fill.argtypes = [vp, i64, vp] + grid + [i32, vp, i64, vp, vp, vp, vp]
    L.btsbot_grid_knn.restype = i32
    L.btsbot_grid_knn.argtypes = [vp, i64, i32] + grid + [vp, vp, vp]
    L.btsbot_layout_smooth_knn.restype = i32
    L.btsbot_layout_smooth_knn.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp]
    L.btsbot_layout_symmetrize_workspace.restype = i64
    L.btsbot_layout_symmetrize_workspace.argtypes = [i64, i32]
    L.btsbot_layout_symmetrize.restype = i32
    L.btsbot_layout_symmetrize.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, vp]
    L.btsbot_layout_init.restype = i32
    L.btsbot_layout_init.argtypes = [vp, i64, C.c_uint64, i32, vp]
    L.btsbot_layout_epochs.restype = i32
    L.btsbot_layout_epochs.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, f32, f32, C.c_uint64, i32, f32, i32, vp]
    L.btsbot_layout_smooth_knn_query.restype = i32
    L.btsbot_layout_smooth_knn_query.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.btsbot_layout_transform.restype = i32
    L.btsbot_layout_transform.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, i32, i32, i32, f32, f32, C.c_uint64, i32, f32, i32,
                                          vp]
    L.btsbot_lof_fit.restype = i32
    L.btsbot_lof_fit.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.btsbot_lof_score.restype = i32
    L.btsbot_lof_score.argtypes = [vp, vp, i64, i32, vp, vp, i64, vp, vp, vp]
    L.btsbot_knn_graph_merge.restype = i32
    L.btsbot_knn_graph_merge.argtypes = [vp, vp, i64, i32, i64, vp, vp, vp, i64, vp, i64, i32, vp, i64, vp, vp, vp]
    L.btsbot_knn_graph_compact.restype = i32
    L.btsbot_knn_graph_compact.argtypes = [vp, vp, i64, i32, i64, vp, vp, vp, i64, i64, i32, vp, vp, vp]
    L.btsbot_kmeans_workspace.restype = i64
    L.btsbot_kmeans_workspace.argtypes = [i64, i32, i32]
    L.btsbot_kmeans_update.restype = i32
    L.btsbot_kmeans_update.argtypes = [vp, i64, i32, vp, vp, i32, vp, vp, vp, i64, vp]
    L.btsbot_ivf_list_rows.restype = i64
    L.btsbot_ivf_list_rows.argtypes = [i64, i32]
    L.btsbot_ivf_layout.restype = i32
    L.btsbot_ivf_layout.argtypes = [vp, i64, i32, vp, vp, i32, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.btsbot_ivf_workspace.restype = i64
    L.btsbot_ivf_workspace.argtypes = [i64, i32, i32, i32, i32]
    L.btsbot_ivf_query.restype = i32
    L.btsbot_ivf_query.argtypes = [vp, i64, vp, i64, i32, i32, vp, i32, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, i64, vp]
    L.btsbot_ivf_layout_groups.restype = i32
    L.btsbot_ivf_layout_groups.argtypes = [vp, i64, i32, vp, i64, vp, vp]
    L.btsbot_ivf_workspace_grouped.restype = i64
    L.btsbot_ivf_workspace_grouped.argtypes = [i64, i32, i32, i32, i32, i32]
    L.btsbot_ivf_query_grouped.restype = i32
    L.btsbot_ivf_query_grouped.argtypes = L.btsbot_ivf_query.argtypes + [vp, vp, i32]
    L.btsbot_mst_offer_knn.restype = i32
    L.btsbot_mst_offer_knn.argtypes = [vp, vp, i64, i32, vp, vp, i32, f32, vp, vp, vp, vp]
    L.btsbot_mst_offer_csr.restype = i32
    L.btsbot_mst_offer_csr.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp]
    L.btsbot_mst_merge.restype = i32
    L.btsbot_mst_merge.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.btsbot_hdbscan_tree.restype = i32
    L.btsbot_hdbscan_tree.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]
    L.btsbot_hdbscan_model.restype = i32
    L.btsbot_hdbscan_model.argtypes = [vp, vp, i64, i64, i32, i32, i32] + [vp] * 8 + [i64, vp, vp]
    L.btsbot_cluster_offer_knn.restype = i32
    L.btsbot_cluster_offer_knn.argtypes = [vp, vp, i64, i32, i64, i32, vp, vp, i32, f32, vp, vp, vp, vp, vp]
    L.btsbot_cluster_offer_csr.restype = i32
    L.btsbot_cluster_offer_csr.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp]
    L.btsbot_cluster_assign.restype = i32
    L.btsbot_cluster_assign.argtypes = [vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, C.c_double] + [vp] * 7
    L.btsbot_eval_metrics.restype = i32
    L.btsbot_eval_metrics.argtypes = [vp, vp, f32, i64, vp, vp]
    if L.btsbot_abi_version() != ABI_VERSION:
        raise BtsbotHipError(f"ABI mismatch: library {L.btsbot_abi_version()} vs binding {ABI_VERSION}")
    _lib = L
    return L


def check(status: int, what: str) -> int:
    if status < 0:
        msg = lib().btsbot_last_error().decode("utf-8", "replace")
        raise BtsbotHipError(f"{what} failed ({status}): {msg}")
    return status


def ptr(t) -> C.c_void_p:
    """The device pointer of a tensor as a C argument; NULL for ``None`` and for a tensor without elements."""
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def stream(device) -> C.c_void_p:
    """The caller's current stream on ``device`` as a C argument."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_config(wiring: str, precision: str, depths, dims, head_norm: bool, n_meta: int,
                meta_fc1: int, meta_fc2: int, comb_fc1: int, comb_fc2: int,
                meta_dropout: float, comb_dropout: float, image_size: int = 63) -> Config:
    if precision not in PRECISION:
        raise ValueError(f"precision must be one of {sorted(set(PRECISION))}, got {precision!r}")
    cfg = Config()
    cfg.abi_version = ABI_VERSION
    cfg.wiring = WIRING[wiring]
    cfg.precision = PRECISION[precision]
    cfg.depths = (C.c_int32 * 4)(*depths)
    cfg.dims = (C.c_int32 * 4)(*dims)
    cfg.image_size = image_size
    cfg.head_norm = int(head_norm)
    cfg.n_meta = n_meta
    cfg.meta_fc1, cfg.meta_fc2 = meta_fc1, meta_fc2
    cfg.comb_fc1, cfg.comb_fc2 = comb_fc1, comb_fc2
    cfg.meta_dropout, cfg.comb_dropout = meta_dropout, comb_dropout
    return cfg


class Handle:
    """Owns one btsbot_handle."""

    def __init__(self, cfg: Config):
        self._h = C.c_void_p()
        check(lib().btsbot_create(C.byref(cfg), C.byref(self._h)), "btsbot_create")

    @property
    def ptr(self):
        return self._h

    def params(self):
        L = lib()
        out = []
        info = ParamInfo()
        for i in range(L.btsbot_param_count(self._h)):
            check(L.btsbot_param_info_at(self._h, i, C.byref(info)), "btsbot_param_info_at")
            shape = tuple(info.shape[k] for k in range(info.ndim))
            out.append((info.name.decode(), int(info.offset), int(info.numel), shape,
                        bool(info.is_buffer)))
        return out

    def param_floats(self) -> int:
        return int(lib().btsbot_param_floats(self._h))

    def close(self):
        if self._h:
            lib().btsbot_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
