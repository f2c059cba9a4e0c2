"""ctypes binding of libpointseg_hip.so -- the only door between the Python host code and the HIP kernels.

The signatures below are include/pointseg.h and pointseg_train_ops.h verbatim (PROTOTYPES) and include/pointseg_prepare.h
(PREPARE_PROTOTYPES), include/pointseg_postprocess.h (POSTPROCESS_PROTOTYPES), include/pointseg_saliency.h
(SALIENCY_PROTOTYPES), include/pointseg_saliency_train.h (SALIENCY_TRAIN_PROTOTYPES), include/pointseg_saliency_attention.h
(SALIENCY_ATTENTION_PROTOTYPES), include/pointseg_saliency_data.h (SALIENCY_DATA_PROTOTYPES), include/pointseg_saliency_step.h
(SALIENCY_STEP_PROTOTYPES), include/pointseg_saliency_step_precision.h (SALIENCY_STEP_PRECISION_PROTOTYPES) and
include/pointseg_saliency_precision.h (SALIENCY_PRECISION_PROTOTYPES), include/pointseg_saliency_map.h (SALIENCY_MAP_PROTOTYPES) and
include/pointseg_saliency_view.h (SALIENCY_VIEW_PROTOTYPES), include/pointseg_forward_precision.h (FORWARD_PRECISION_PROTOTYPES) and
include/pointseg_train_loss.h (TRAIN_LOSS_PROTOTYPES).
The library is built in-tree by compile_op.sh (csrc/Makefile); a missing library is a hard error: there is no CPU fallback anywhere in this package.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpointseg_hip.so")
PS_ABI_VERSION = 7  # include/pointseg.h
PS_VOLUME_I16, PS_VOLUME_F32 = 1, 2
PS_VOLUME_U8 = 3  # include/pointseg_prepare.h

PS_MAX_LAYERS = 8
c_f32p = ctypes.POINTER(ctypes.c_float)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_vp = ctypes.c_void_p


class PsPyramid(ctypes.Structure):
    _fields_ = [
        ("num_layers", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("n", ctypes.c_int64 * (PS_MAX_LAYERS + 1)),
        ("xyz", c_vp * PS_MAX_LAYERS),
        ("neigh_idx", c_vp * PS_MAX_LAYERS),
        ("sub_idx", c_vp * PS_MAX_LAYERS),
        ("interp_idx", c_vp * PS_MAX_LAYERS),
        ("order", c_vp * PS_MAX_LAYERS),
        ("built", ctypes.c_uint64),  # ps_pyramid_build's stamp: sub_idx IS the prefix of neigh_idx (0 = caller-filled, compared every step)
    ]


class PsRandlaConfig(ctypes.Structure):
    _fields_ = [
        ("num_layers", ctypes.c_int32),
        ("k_n", ctypes.c_int32),
        ("num_classes", ctypes.c_int32),
        ("in_channels", ctypes.c_int32),
        ("d_out", ctypes.c_int32 * PS_MAX_LAYERS),
    ]


class PsTrainOptions(ctypes.Structure):
    _fields_ = [
        ("learning_rate", ctypes.c_float),
        ("keep_prob", ctypes.c_float),
        ("mlp_bf16", ctypes.c_int32),
        ("fused_att", ctypes.c_int32),
        ("fused_locse", ctypes.c_int32),
        ("num_ignored", ctypes.c_int32),
        ("ignored_label_inds", ctypes.c_int32 * 8),
        ("deterministic", ctypes.c_int32),
        ("fused_convbn", ctypes.c_int32),
        ("overlap_wgrad", ctypes.c_int32),
        ("act_bf16", ctypes.c_int32),
    ]


class PsVolumeSampleArgs(ctypes.Structure):
    _fields_ = [
        ("volume", c_vp),
        ("volume_dtype", ctypes.c_int32),
        ("dilate", ctypes.c_int32),
        ("X", ctypes.c_int64),
        ("Y", ctypes.c_int64),
        ("Z", ctypes.c_int64),
        ("mask", c_vp),
        ("probs", c_vp),
        ("probs_C", ctypes.c_int32),
        ("probs_channel", ctypes.c_int32),
        ("threshold", ctypes.c_float),
        ("loops", ctypes.c_int32),
        ("truth", c_vp),
        ("label_src", c_vp),
        ("N", ctypes.c_int64),
        ("seed", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("out_mask", c_vp),
        ("out_stats", c_vp),
        ("out_positives", c_vp),
        ("out_xyz", c_vp),
        ("out_features", c_vp),
        ("out_labels", c_vp),
        ("out_origin", c_vp),
        ("out_idx", c_vp),
        ("scratch", c_vp),
        ("scratch_bytes", ctypes.c_int64),
    ]


# int (*ps_allreduce_fn)(void* user, void* buf, int64_t count, int dtype, void* hip_stream)
PS_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p)


class PsTimingRow(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("ms", ctypes.c_double), ("launches", ctypes.c_int64)]


# name -> (restype, argtypes); every symbol include/pointseg.h declares
PROTOTYPES = {
    "ps_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_vp)]),
    "ps_destroy": (ctypes.c_int, [c_vp]),
    "ps_set_stream": (ctypes.c_int, [c_vp, c_vp]),
    "ps_synchronize": (ctypes.c_int, [c_vp]),
    "ps_set_deferred_checks": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_last_error": (ctypes.c_char_p, []),
    "ps_version": (ctypes.c_char_p, []),
    "ps_abi_version": (ctypes.c_int, []),
    "ps_set_train_gemm_bf16": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_set_train_act_bf16": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_set_att_bf16x3": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_set_train_gemm_b3": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_timing_begin": (ctypes.c_int, [c_vp]),
    "ps_timing_select": (ctypes.c_int, [c_vp, ctypes.c_char_p]),
    "ps_timing_end": (ctypes.c_int, [c_vp, ctypes.POINTER(PsTimingRow), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "ps_knn_batch": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp, ctypes.c_int]),
    "ps_knn_batch_i64": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp, ctypes.c_int]),
    "ps_pyramid_build": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, c_i32p, ctypes.c_int32,
                                        ctypes.POINTER(PsPyramid)]),
    "ps_grid_subsample": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_float,
                                         c_i64p, c_vp, c_vp, c_vp]),
    "ps_randla_create": (ctypes.c_int, [c_vp, ctypes.POINTER(PsRandlaConfig), ctypes.POINTER(c_vp)]),
    "ps_randla_destroy": (ctypes.c_int, [c_vp]),
    "ps_randla_weight_count": (ctypes.c_int64, [c_vp]),
    "ps_randla_set_weights": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64]),
    "ps_randla_forward": (ctypes.c_int, [c_vp, ctypes.POINTER(PsPyramid), c_vp, c_vp]),
    "ps_randla_tap": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_randla_keep_taps": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_op_gather_neighbour": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp]),
    "ps_op_relative_pos_encoding": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp]),
    "ps_op_random_sample": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp]),
    "ps_op_nearest_interpolation": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 4 + [c_vp]),
    "ps_op_conv1x1": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int, c_vp]),
    "ps_op_att_pool": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp]),
    "ps_op_probs_to_volume": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp] + [ctypes.c_int64] * 4 + [c_vp, c_vp]),
    "ps_op_linear_wgrad": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_op_bn_train_fwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int] + [c_vp] * 5),
    "ps_op_bn_train_bwd": (ctypes.c_int, [c_vp] * 7 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [c_vp] * 3),
    "ps_volume_to_cloud": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int64)] + [c_vp] * 4),
    "ps_volume_to_cloud_dev": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int64)] + [c_vp] * 4),
    "ps_grid_subsample_dev": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_float, ctypes.c_int64,
                                             c_i64p, c_vp, c_vp, c_vp]),
    "ps_op_half_to_float": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp]),
    # evaluation (csrc/metrics.hip)
    "ps_confusion_accumulate": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp]),
    "ps_probs_to_labels": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_i32p, c_vp]),
    "ps_seg_metrics": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.c_int32, c_vp, ctypes.c_int64, c_i64p, ctypes.POINTER(ctypes.c_double)]),
    "ps_seg_metrics_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64] * 3 + [ctypes.c_int32]),
    # training batches from resident clouds (csrc/cloud_sample.hip)
    "ps_cloud_positive_counts": (ctypes.c_int, [c_vp, c_vp, c_i64p, ctypes.c_int64, c_i64p]),
    "ps_cloud_sample": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_i64p, ctypes.c_int64, c_i64p, c_i32p, ctypes.c_int32, ctypes.c_int64,
                                       ctypes.c_uint32, c_vp, c_vp, c_vp, c_vp]),
    # volume -> the network's clouds, Pancreas form (csrc/volume_sample.hip)
    "ps_volume_sample": (ctypes.c_int, [c_vp, ctypes.POINTER(PsVolumeSampleArgs)]),
    "ps_op_bn_train_sums": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_bn_train_apply": (ctypes.c_int, [c_vp] * 5 + [ctypes.c_int64] * 3 + [ctypes.c_float, ctypes.c_int] + [c_vp] * 4),
    "ps_op_bn_train_bwd_sums": (ctypes.c_int, [c_vp] * 7 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [c_vp] * 2),
    "ps_op_bn_train_bwd_apply": (ctypes.c_int, [c_vp] * 9 + [ctypes.c_int64] * 3 + [ctypes.c_int, c_vp]),
    "ps_op_scatter_add_rows": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 4 + [c_vp]),
    "ps_op_softmax_pool_fwd": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_op_softmax_pool_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_op_softmax_pool_bwd_scores": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_op_att_pool_train_supported": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "ps_op_att_pool_train_supported_ex": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "ps_op_att_pool_gemm_supported": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "ps_op_att_pool_gemm_fwd": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp] + [ctypes.c_int64] * 3 + [c_vp]),
    "ps_op_att_pool_gemm_bwd": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, ctypes.c_int64, ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_op_att_pool_gemm_fwd_split": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp,
                                                     ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_att_pool_gemm_bwd_split": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, c_vp,
                                                     ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_op_linear_wgrad_split": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64,
                                                c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_att_pool_train_fwd": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp] + [ctypes.c_int64] * 3 + [c_vp]),
    "ps_op_att_pool_train_bwd": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, ctypes.c_int64, c_vp]),
    "ps_op_conv_bn_train_supported": (ctypes.c_int, [ctypes.c_int64]),
    "ps_op_conv_bn_train_sums": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_conv_bn_train_apply": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp,
                                                 ctypes.c_int64]),
    "ps_op_conv_bn_train_bwd_sums": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                    ctypes.c_int64, c_vp]),
    "ps_op_conv_bn_train_bwd_apply": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                     c_vp, c_vp, ctypes.c_int64, ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_op_conv_bn_train_bwd_sums2": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                     ctypes.c_int64, c_vp]),
    "ps_op_conv_bn_train_bwd_apply_w": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                       ctypes.c_float, c_vp, ctypes.c_int64, ctypes.c_int, c_vp, ctypes.c_int64, c_vp, c_vp]),
    "ps_op_convbn_train_supported": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "ps_op_convbn_train_sums": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_convbn_train_apply": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp,
                                                ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_op_convbn_train_apply_add": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp,
                                                    c_vp, ctypes.c_int64, c_vp, ctypes.c_int64]),
    "ps_op_convbn_train_bwd_sums": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp,
                                                   c_vp, ctypes.c_int, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_convbn_train_bwd_apply": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp,
                                                    c_vp, ctypes.c_int, c_vp, ctypes.c_float, c_vp, ctypes.c_int64, ctypes.c_int, c_vp, ctypes.c_int64, c_vp,
                                                    c_vp]),
    "ps_op_locse_train_supported": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "ps_op_locse_train_sums": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_locse_train_apply": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, c_vp, c_vp,
                                               c_vp, c_vp, ctypes.c_int64]),
    "ps_op_locse_train_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, c_vp, c_vp,
                                             c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_att_pool_train_fwd_split": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_att_pool_train_bwd_split": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64,
                                                      c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_inverse_index_workspace": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "ps_op_inverse_index": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp]),
    "ps_op_gather_reduce_rows": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int]),
    "ps_op_gather_reduce_rows_ordered": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int,
                                                        c_vp, ctypes.c_int64]),
    "ps_op_random_sample_bwd_inv": (ctypes.c_int, [c_vp] * 7 + [ctypes.c_int64] * 5 + [c_vp, c_vp, c_vp]),
    "ps_op_random_sample_ties": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp, c_vp]),
    "ps_op_att_pool_train_bwd_split_rows": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, c_vp,
                                                           ctypes.c_int64, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_random_sample_bwd": (ctypes.c_int, [c_vp] * 5 + [ctypes.c_int64] * 5 + [c_vp]),
    "ps_op_add_lrelu": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_add_lrelu_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_axpy": (ctypes.c_int, [c_vp, ctypes.c_float, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_mul": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]),
    "ps_op_weighted_ce": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp]),
    "ps_op_adam": (ctypes.c_int, [c_vp] * 5 + [ctypes.c_int64] + [ctypes.c_float] * 4 + [ctypes.c_int64]),
    "ps_op_dropout": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, c_vp, c_vp]),
    # row-strided / accumulating variants (the training step's concat buffers, include/pointseg.h)
    "ps_op_gather_neighbour_ex": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 5 + [c_vp, ctypes.c_int64]),
    "ps_op_conv1x1_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int64]),
    "ps_op_linear_wgrad_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64] + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_op_bn_train_fwd_ex": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int, c_vp, ctypes.c_int64]
                              + [c_vp] * 4),
    "ps_op_bn_train_fwd_mov": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int, c_vp, ctypes.c_int64]
                               + [c_vp] * 6 + [ctypes.c_float]),
    "ps_op_bn_train_bwd_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64] + [c_vp] * 5 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [c_vp] * 3),
    "ps_op_bn_train_apply_ex": (ctypes.c_int, [c_vp] * 5 + [ctypes.c_int64] * 3 + [ctypes.c_float, ctypes.c_int, c_vp, ctypes.c_int64] + [c_vp] * 3),
    "ps_op_bn_train_bwd_sums_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64] + [c_vp] * 5 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [c_vp] * 2),
    "ps_op_bn_train_bwd_apply_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64] + [c_vp] * 7 + [ctypes.c_int64] * 3 + [ctypes.c_int, c_vp]),
    "ps_op_scatter_add_rows_ex": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int64, c_vp] + [ctypes.c_int64] * 4 + [c_vp]),
    # the training step behind one call (csrc/trainer.hip)
    "ps_trainer_create": (ctypes.c_int, [c_vp, ctypes.POINTER(PsRandlaConfig), ctypes.POINTER(PsTrainOptions), ctypes.POINTER(c_vp)]),
    "ps_trainer_destroy": (ctypes.c_int, [c_vp]),
    "ps_trainer_param_count": (ctypes.c_int64, [c_vp]),
    "ps_trainer_buffer_count": (ctypes.c_int64, [c_vp]),
    "ps_trainer_layout_rows": (ctypes.c_int, [c_vp]),
    "ps_trainer_layout": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, c_i64p, c_i64p, c_i64p, ctypes.POINTER(ctypes.c_int)]),
    "ps_trainer_bind": (ctypes.c_int, [c_vp] * 6),
    "ps_trainer_set_collective": (ctypes.c_int, [c_vp, PS_ALLREDUCE_FN, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "ps_trainer_set_options": (ctypes.c_int, [c_vp, ctypes.POINTER(PsTrainOptions)]),
    "ps_trainer_set_step": (ctypes.c_int, [c_vp, ctypes.c_int64]),
    "ps_trainer_get_step": (ctypes.c_int64, [c_vp]),
    "ps_trainer_pool_peak_bytes": (ctypes.c_int64, [c_vp]),
    "ps_trainer_set_profile": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "ps_trainer_profile": (ctypes.c_int, [c_vp, ctypes.POINTER(PsTimingRow), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "ps_trainer_collective_stats": (ctypes.c_int, [c_vp, c_i64p, c_i64p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "ps_randla_backward": (ctypes.c_int, [c_vp, ctypes.POINTER(PsPyramid), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "ps_randla_train_step": (ctypes.c_int, [c_vp, ctypes.POINTER(PsPyramid), c_vp, c_vp, c_vp, c_vp, c_vp]),
}

# every symbol include/pointseg_prepare.h declares (dataset preparation in front of the entry points above; csrc/resample.hip)
PREPARE_PROTOTYPES = {
    "ps_volume_zoom": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int32] + [ctypes.c_int64] * 3 + [ctypes.c_int32] + [ctypes.c_int64] * 3
                       + [ctypes.c_uint32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, c_vp, c_vp, c_i64p]),
}

# every symbol include/pointseg_postprocess.h declares (the clean-up of a predicted label volume; csrc/postprocess.hip)
PS_MORPH_DILATE, PS_MORPH_ERODE, PS_MORPH_CLOSE, PS_MORPH_OPEN = 1, 2, 3, 4
PS_KEEP_ABOVE, PS_KEEP_LARGEST_TWO, PS_KEEP_OVERLAP = 1, 2, 3
POSTPROCESS_PROTOTYPES = {
    "ps_label_components": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int32, ctypes.c_int32] + [c_vp] * 5 + [c_i64p]),
    "ps_binary_morph": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int32] * 3 + [c_vp, c_vp, c_i64p]),
    "ps_keep_components": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, c_vp, c_vp, c_vp, c_i64p]),
    "ps_fill_holes": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp, c_i64p]),
    "ps_brats_postprocess": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [ctypes.c_int64, c_vp, c_vp, c_i64p]),
}


class PsSaliencyTaps(ctypes.Structure):
    _fields_ = [("down4", c_vp), ("c345", c_vp), ("sa", c_vp), ("c12", c_vp)]


# every symbol include/pointseg_saliency.h declares (the saliency attention network and its window average; csrc/conv3d.hip, csrc/saliency.hip)
SALIENCY_PROTOTYPES = {
    "ps_conv3d": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 6 + [ctypes.c_int32, c_vp, c_vp] + [ctypes.c_int32] * 3 + [ctypes.c_int64]
                  + [ctypes.c_int32] * 2 + [c_vp]),
    "ps_instance_norm_relu": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, c_vp, ctypes.c_float, c_vp, c_vp, c_i64p]),
    "ps_saliency_weight_count": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "ps_saliency_forward": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 6 + [c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.POINTER(PsSaliencyTaps), c_vp, c_i64p]),
    "ps_saliency_accumulate": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 10 + [c_vp, c_vp]),
    "ps_saliency_finish": (ctypes.c_int, [c_vp, c_vp, c_vp] + [ctypes.c_int64] * 4 + [c_vp]),
}

# every symbol include/pointseg_saliency_precision.h declares (ps_conv3d and ps_saliency_forward with a choice of arithmetic for the
# convolutions; csrc/conv3d_bf16.hip): the arguments of the entries they extend, then the precision
PS_PREC_FP32, PS_PREC_BF16X3, PS_PREC_BF16 = 0, 1, 2
SALIENCY_PRECISIONS = {"fp32": PS_PREC_FP32, "bf16x3": PS_PREC_BF16X3, "bf16": PS_PREC_BF16}
SALIENCY_PRECISION_PROTOTYPES = {
    "ps_conv3d_prec": (ctypes.c_int, SALIENCY_PROTOTYPES["ps_conv3d"][1] + [ctypes.c_int32]),
    "ps_saliency_forward_prec": (ctypes.c_int, SALIENCY_PROTOTYPES["ps_saliency_forward"][1] + [ctypes.c_int32]),
}

# every symbol include/pointseg_saliency_train.h declares (the gradients of ps_conv3d and ps_instance_norm_relu; csrc/conv3d_train.hip, csrc/saliency_train.hip)
_CONV_GEOMETRY = [ctypes.c_int64] * 6 + [ctypes.c_int32] * 4 + [ctypes.c_int64] + [ctypes.c_int32] * 2  # B Ds Hs Ws C1 C2 up kd kh kw C_out stride dilation
SALIENCY_TRAIN_PROTOTYPES = {
    "ps_conv3d_bwd_data": (ctypes.c_int, [c_vp, c_vp, c_vp] + _CONV_GEOMETRY + [c_vp, c_vp, c_vp, c_i64p]),
    "ps_conv3d_bwd_weight": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp] + _CONV_GEOMETRY + [c_vp, c_vp, c_vp, c_i64p]),
    "ps_instance_norm_relu_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp] + [ctypes.c_int64] * 3 + [c_vp, ctypes.c_float, c_vp, c_vp, c_vp, c_vp, c_i64p]),
}

# every symbol include/pointseg_saliency_train_precision.h declares (the convolution's two gradients with a choice of arithmetic;
# csrc/conv3d_train.hip, csrc/conv3d_bf16.hip, csrc/conv3d_train_bf16.hip): the arguments of the entries they extend, then the precision
SALIENCY_TRAIN_PRECISION_PROTOTYPES = {
    "ps_conv3d_bwd_data_prec": (ctypes.c_int, SALIENCY_TRAIN_PROTOTYPES["ps_conv3d_bwd_data"][1] + [ctypes.c_int32]),
    "ps_conv3d_bwd_weight_prec": (ctypes.c_int, SALIENCY_TRAIN_PROTOTYPES["ps_conv3d_bwd_weight"][1] + [ctypes.c_int32]),
}

# every symbol include/pointseg_saliency_attention.h declares (the channel attention, the spatial gate and softmax + Dice, each with its
# gradient; csrc/saliency_train.hip)
SALIENCY_ATTENTION_PROTOTYPES = {
    "ps_channel_attention": (ctypes.c_int, [c_vp, c_vp] + [ctypes.c_int64] * 4 + [c_vp] * 8 + [c_vp, c_i64p]),
    "ps_channel_attention_bwd": (ctypes.c_int, [c_vp] * 8 + [ctypes.c_int64] * 4 + [c_vp] * 5 + [c_vp, c_i64p]),
    "ps_spatial_gate": (ctypes.c_int, [c_vp] * 5 + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_spatial_gate_bwd": (ctypes.c_int, [c_vp] * 4 + [ctypes.c_int64] * 3 + [c_vp, c_vp]),
    "ps_softmax_dice_loss": (ctypes.c_int, [c_vp] * 4 + [ctypes.c_int64] * 3 + [c_vp, c_vp, c_vp, c_i64p]),
    "ps_softmax_dice_loss_bwd": (ctypes.c_int, [c_vp] * 6 + [ctypes.c_int64] * 3 + [c_vp]),
}

# every symbol include/pointseg_saliency_data.h declares (volumes prepared and kept on the device, training patches drawn from them;
# csrc/saliency_data.hip)
PS_PATCH_RANDOM, PS_PATCH_ALL_POSITIVE, PS_PATCH_ONE_POSITIVE = 0, 1, 2
PS_PATCH_MAX_B, PS_PATCH_MAX_T, PS_PATCH_MAX_C = 64, 16, 16
SALIENCY_DATA_PROTOTYPES = {
    "ps_saliency_brats_measure": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int32] + [ctypes.c_int64] * 3 + [ctypes.c_int32, c_i64p, ctypes.POINTER(ctypes.c_double)]),
    "ps_saliency_brats_apply": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int32] + [ctypes.c_int64] * 3 + [ctypes.c_int32, c_i64p, ctypes.POINTER(ctypes.c_double)]
                                + [c_vp] * 3),
    "ps_saliency_pancreas_prepare": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int32, ctypes.c_int64] + [c_vp] * 4),
    "ps_patch_sample": (ctypes.c_int, [c_vp, ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_i64p, ctypes.c_int64, ctypes.c_int32, c_i32p,
                                       ctypes.c_int32, ctypes.c_int32, c_i64p, ctypes.c_uint32, ctypes.c_int32] + [c_vp] * 4),
}



class PsSaliencyStepOptions(ctypes.Structure):
    _fields_ = [("allreduce", PS_ALLREDUCE_FN), ("user", c_vp), ("world_size", ctypes.c_int32), ("momentum", ctypes.c_float), ("l2", ctypes.c_float)]


# every symbol include/pointseg_saliency_step.h declares (the saliency network's training step behind one call; csrc/saliency_step.hip)
_PATCH_SHAPE = [ctypes.c_int64] * 6  # B D H W C_in num_classes
SALIENCY_STEP_PROTOTYPES = {
    "ps_saliency_backward": (ctypes.c_int, [c_vp] * 4 + _PATCH_SHAPE + [c_vp, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_i64p]),
    "ps_saliency_sgd_update": (ctypes.c_int, [c_vp] * 4 + [ctypes.c_int64] * 3 + [ctypes.c_float] * 4),
    "ps_saliency_train_step": (ctypes.c_int, [c_vp] * 4 + _PATCH_SHAPE + [c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_float,
                                                                         ctypes.POINTER(PsSaliencyStepOptions), c_vp, c_vp, c_vp, c_i64p]),
}

# every symbol include/pointseg_saliency_mixup.h declares (config.MIXUP: mixed batches, the soft-label Dice loss, the step on soft labels;
# csrc/saliency_data.hip, csrc/saliency_train.hip, csrc/saliency_step.hip)
SALIENCY_MIXUP_PROTOTYPES = {
    "ps_patch_sample_mixup": (ctypes.c_int, [c_vp, ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_i64p, ctypes.c_int64, ctypes.c_int32, c_i32p,
                                             ctypes.c_int32, ctypes.c_int32, c_i64p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_double)] + [c_vp] * 4),
    "ps_softmax_dice_soft_loss": SALIENCY_ATTENTION_PROTOTYPES["ps_softmax_dice_loss"],
    "ps_softmax_dice_soft_loss_bwd": SALIENCY_ATTENTION_PROTOTYPES["ps_softmax_dice_loss_bwd"],
    "ps_saliency_backward_soft": SALIENCY_STEP_PROTOTYPES["ps_saliency_backward"],
    "ps_saliency_train_step_soft": SALIENCY_STEP_PROTOTYPES["ps_saliency_train_step"],
}

# every symbol include/pointseg_saliency_step_precision.h declares (the one-call step with a precision per role of its convolutions;
# csrc/saliency_step.hip): the arguments of the entries they extend, then soft_labels and the forward's, the data gradient's and the
# weight gradient's precision
SALIENCY_STEP_PRECISION_PROTOTYPES = {
    "ps_saliency_backward_prec": (ctypes.c_int, SALIENCY_STEP_PROTOTYPES["ps_saliency_backward"][1] + [ctypes.c_int32] * 4),
    "ps_saliency_train_step_prec": (ctypes.c_int, SALIENCY_STEP_PROTOTYPES["ps_saliency_train_step"][1] + [ctypes.c_int32] * 4),
}

# every symbol include/pointseg_saliency_map.h declares (the saliency map of a whole volume behind one call: views, flip, fusion;
# csrc/saliency_map.hip)
PS_VIEW_AXIAL, PS_VIEW_SAGITTAL, PS_VIEW_CORONAL = 0, 1, 2
SALIENCY_VIEWS = {"axial": PS_VIEW_AXIAL, "sagittal": PS_VIEW_SAGITTAL, "coronal": PS_VIEW_CORONAL}
PS_VOLUME_CDHW, PS_VOLUME_DHWC = 0, 1
SALIENCY_MAP_PROTOTYPES = {
    "ps_saliency_map": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int32] + [ctypes.c_int64] * 5 + [ctypes.c_int32, c_i32p, ctypes.POINTER(c_vp), ctypes.c_int64, c_i64p,
                                       c_i64p] + [ctypes.c_int32] * 3 + [c_vp, c_vp, c_i64p]),
}

# every symbol include/pointseg_saliency_view.h declares (the two patch samplers through an anatomical view, with the per-sample flip;
# csrc/saliency_data.hip): the arguments of the entries they extend, with view and flip in front of the outputs
SALIENCY_VIEW_PROTOTYPES = {
    "ps_patch_sample_view": (ctypes.c_int, SALIENCY_DATA_PROTOTYPES["ps_patch_sample"][1][:-4] + [ctypes.c_int32, c_i32p] + [c_vp] * 4),
    "ps_patch_sample_mixup_view": (ctypes.c_int, SALIENCY_MIXUP_PROTOTYPES["ps_patch_sample_mixup"][1][:-4] + [ctypes.c_int32, c_i32p] + [c_vp] * 4),
}

# every symbol include/pointseg_forward_precision.h declares (the point network's forward on one plane of rounded bfloat16 operands;
# csrc/randla.hip): a per-network switch over the PS_PREC_* values above, of which the forward takes two
FORWARD_PRECISIONS = {"bf16x3": PS_PREC_BF16X3, "bf16": PS_PREC_BF16}
FORWARD_PRECISION_PROTOTYPES = {
    "ps_randla_set_precision": (ctypes.c_int, [c_vp, ctypes.c_int32]),
    "ps_randla_get_precision": (ctypes.c_int, [c_vp, c_i32p]),
}

# every symbol include/pointseg_train_loss.h declares (the objective of the point network's training step -- cross-entropy or the
# reference's two Dice losses -- and the step's accuracy; csrc/point_loss.hip, csrc/trainer.hip)
PS_LOSS_CE, PS_LOSS_DICE, PS_LOSS_DICE_WEIGHTED = 0, 1, 2
TRAIN_LOSSES = {"ce": PS_LOSS_CE, "dice": PS_LOSS_DICE, "dice_weighted": PS_LOSS_DICE_WEIGHTED}
_STEP_LOSS = [c_vp, ctypes.POINTER(PsPyramid), c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp]
TRAIN_LOSS_PROTOTYPES = {
    "ps_op_dice_sums": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_op_dice_from_sums": (ctypes.c_int, [c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, ctypes.c_float, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp]),
    "ps_op_top1_counts": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp]),
    "ps_randla_backward_loss": (ctypes.c_int, _STEP_LOSS),
    "ps_randla_train_step_loss": (ctypes.c_int, _STEP_LOSS),
}

_lib = None


class PointSegError(RuntimeError):
    pass


def lib():
    """The loaded library.  Raises if it has not been built -- never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PointSegError("libpointseg_hip.so is missing: build it with `sh point-unet_amd/compile_op.sh` "
                                "(or __graft_entry__.build()); there is no CPU fallback")
        try:  # share torch's HIP runtime (same SONAME libamdhip64.so.7) when torch is in the process
            import torch  # noqa: F401
        except Exception:  # pragma: no cover
            pass
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(PROTOTYPES.items()) + list(PREPARE_PROTOTYPES.items()) + list(POSTPROCESS_PROTOTYPES.items())
                                  + list(SALIENCY_PROTOTYPES.items()) + list(SALIENCY_PRECISION_PROTOTYPES.items())
                                  + list(SALIENCY_TRAIN_PROTOTYPES.items()) + list(SALIENCY_TRAIN_PRECISION_PROTOTYPES.items())
                                  + list(SALIENCY_ATTENTION_PROTOTYPES.items()) + list(SALIENCY_DATA_PROTOTYPES.items())
                                  + list(SALIENCY_STEP_PROTOTYPES.items()) + list(SALIENCY_MIXUP_PROTOTYPES.items())
                                  + list(SALIENCY_STEP_PRECISION_PROTOTYPES.items()) + list(SALIENCY_MAP_PROTOTYPES.items())
                                  + list(SALIENCY_VIEW_PROTOTYPES.items()) + list(FORWARD_PRECISION_PROTOTYPES.items())
                                  + list(TRAIN_LOSS_PROTOTYPES.items())):
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.ps_abi_version() != PS_ABI_VERSION:  # (the ctypes Structures below mirror include/pointseg.h at this revision)
            raise PointSegError("libpointseg_hip.so has struct layout revision %d, this package was written against %d: rebuild the library"
                                % (handle.ps_abi_version(), PS_ABI_VERSION))
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise PointSegError("libpointseg_hip: %s (code %d)" % (lib().ps_last_error().decode(), rc))
