"""ctypes binding of ``libhvr_hip.so`` (C ABI: ``include/hvr_hip.h``).

PyTorch is used only for device memory and streams: every wrapper here takes CUDA(ROCm)
tensors, passes ``data_ptr()`` + sizes + the current stream to the C ABI and returns
tensors it allocated with the torch allocator.  There is NO CPU fallback: a missing
library or a CPU tensor raises (the reference's RoIAlign raises ``NotImplementedError`` on
CPU input the same way, ``mmdet/ops/roi_align/roi_align.py:27-28``).
"""
import contextlib
import ctypes
import math
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libhvr_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'hvr_hip.h')

HVR_F32, HVR_BF16, HVR_F16, HVR_F16S = 0, 1, 2, 3
ABI_VERSION = 7
# Split-half tensors (HVR_F16S, include/hvr_hip.h: [32 hi | 32 lo] half groups, 4 bytes per logical element) travel through
# torch as int32 tensors of the LOGICAL shape: element size, strides, row / 32-column slicing, cat, clone and zeros all mean
# the right thing on the container, and nothing but this library ever interprets the bytes.  `SPLIT` is the dtype sentinel
# (`set_compute_dtype(model, native.SPLIT)`).
SPLIT = torch.int32
COMPUTE_DTYPES = (torch.bfloat16, torch.float16, SPLIT, torch.float32)
FUSED_DTYPES = COMPUTE_DTYPES[:3]   # the formats the fused stem and the fused Bottleneck entries have kernels for
DTYPE_NAMES = {torch.bfloat16: 'bf16', torch.float16: 'f16', SPLIT: 'f16x2', torch.float32: 'f32'}
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1

# default operand staging of the MFMA tile engine (0 register-staged, 1 global->LDS DMA)
STAGING = 1   # operand loader of the tile engine: 1 = LDS-DMA (the product path); 0 = register staging, kept as the second loader the
              # kernel tests cross-check (3 x slower); an argument of the C ABI, not an environment switch
# 0 = the library's cost model picks the tile shape; k > 0 forces shape k-1 (tools/kernel_bench.py sweeps)
TILE_HINT = 0


class HvrError(RuntimeError):
    pass


class GemmDesc(ctypes.Structure):
    _fields_ = [('A', ctypes.c_void_p), ('B', ctypes.c_void_p), ('C', ctypes.c_void_p),
                ('M', ctypes.c_int32), ('N', ctypes.c_int32), ('K', ctypes.c_int32),
                ('lda', ctypes.c_int64), ('ldb', ctypes.c_int64), ('ldc', ctypes.c_int64),
                ('bias', ctypes.c_void_p), ('resid', ctypes.c_void_p), ('ldr', ctypes.c_int64),
                ('relu', ctypes.c_int32), ('out_f32', ctypes.c_int32),
                ('dtype', ctypes.c_int32), ('staging', ctypes.c_int32), ('tile_hint', ctypes.c_int32),
                ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('alpha', ctypes.c_float), ('beta', ctypes.c_float)]


class ConvDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
                ('Cin', ctypes.c_int32), ('Cout', ctypes.c_int32), ('KH', ctypes.c_int32),
                ('KW', ctypes.c_int32), ('stride', ctypes.c_int32), ('pad', ctypes.c_int32),
                ('dil', ctypes.c_int32),
                ('bias', ctypes.c_void_p), ('resid', ctypes.c_void_p),
                ('relu', ctypes.c_int32), ('out_f32', ctypes.c_int32),
                ('dtype', ctypes.c_int32), ('staging', ctypes.c_int32), ('tile_hint', ctypes.c_int32),
                ('zero', ctypes.c_void_p), ('ws', ctypes.c_void_p), ('ws_bytes', ctypes.c_size_t), ('alpha', ctypes.c_float),
                ('beta', ctypes.c_float)]


class GConvDesc(ctypes.Structure):          # hvr_gconv_desc
    _fields_ = [('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('y', ctypes.c_void_p), ('bias', ctypes.c_void_p),
                ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('C', ctypes.c_int32),
                ('groups', ctypes.c_int32), ('stride', ctypes.c_int32), ('pad', ctypes.c_int32), ('dil', ctypes.c_int32),
                ('relu', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class Res2ConvDesc(ctypes.Structure):       # hvr_res2_conv_desc
    _fields_ = [('x', ctypes.c_void_p), ('add', ctypes.c_void_p), ('y', ctypes.c_void_p), ('w', ctypes.c_void_p), ('bias', ctypes.c_void_p),
                ('ldx', ctypes.c_int64), ('lda', ctypes.c_int64), ('ldy', ctypes.c_int64),
                ('x_off', ctypes.c_int64), ('add_off', ctypes.c_int64), ('y_off', ctypes.c_int64),
                ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('Wp', ctypes.c_int32),
                ('stride', ctypes.c_int32), ('pad', ctypes.c_int32), ('dil', ctypes.c_int32), ('relu', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class PoolDesc(ctypes.Structure):           # hvr_pool_desc
    _fields_ = [('x', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('ldx', ctypes.c_int64), ('ldy', ctypes.c_int64), ('x_off', ctypes.c_int64), ('y_off', ctypes.c_int64),
                ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('C', ctypes.c_int32), ('k', ctypes.c_int32),
                ('stride', ctypes.c_int32), ('pad', ctypes.c_int32), ('ceil_mode', ctypes.c_int32), ('count_include_pad', ctypes.c_int32),
                ('dtype', ctypes.c_int32)]


class GcbMlp(ctypes.Structure):             # hvr_gcb_mlp
    _fields_ = [(n, ctypes.c_void_p) for n in ('w1', 'b1', 'gamma', 'beta', 'w2t', 'b2')]


class GenAttnDesc(ctypes.Structure):         # hvr_gen_attn_desc
    _fields_ = [(n, ctypes.c_void_p) for n in ('q', 'k', 'v', 'appr_bias', 'px', 'py', 'gx', 'gy', 'o')] + \
               [(n, ctypes.c_int32) for n in ('B', 'heads', 'd', 'H', 'W', 'Hk', 'Wk', 'qk', 'dtype')]


class TailDesc(ctypes.Structure):
    _fields_ = [('h', ctypes.c_void_p), ('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('B', ctypes.c_int32), ('OH', ctypes.c_int32), ('OW', ctypes.c_int32), ('C1', ctypes.c_int32),
                ('H2', ctypes.c_int32), ('W2', ctypes.c_int32), ('C2', ctypes.c_int32), ('stride2', ctypes.c_int32),
                ('Cout', ctypes.c_int32), ('bias', ctypes.c_void_p), ('relu', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class TailNextDesc(ctypes.Structure):
    _fields_ = [('tail', TailDesc), ('resid', ctypes.c_void_p), ('wn', ctypes.c_void_p), ('bias_n', ctypes.c_void_p),
                ('hn', ctypes.c_void_p), ('Cn', ctypes.c_int32), ('alpha', ctypes.c_float), ('beta', ctypes.c_float)]


class TailNextLiveDesc(ctypes.Structure):
    _fields_ = [('next', TailNextDesc), ('live_stride', ctypes.c_int32)]


class CloseSampledDesc(ctypes.Structure):
    _fields_ = [('h', ctypes.c_void_p), ('w', ctypes.c_void_p), ('resid', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('B', ctypes.c_int32), ('OH', ctypes.c_int32), ('OW', ctypes.c_int32), ('C1', ctypes.c_int32),
                ('Cout', ctypes.c_int32), ('RH', ctypes.c_int32), ('RW', ctypes.c_int32), ('rstride', ctypes.c_int32),
                ('bias', ctypes.c_void_p), ('relu', ctypes.c_int32), ('dtype', ctypes.c_int32),
                ('alpha', ctypes.c_float), ('beta', ctypes.c_float)]


class RpnDesc(ctypes.Structure):
    _fields_ = [('cls', ctypes.c_void_p), ('reg', ctypes.c_void_p),
                ('T', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
                ('A', ctypes.c_int32), ('anchor_stride', ctypes.c_int32),
                ('base_anchors', ctypes.c_void_p), ('means', ctypes.c_void_p), ('stds', ctypes.c_void_p),
                ('img_h', ctypes.c_float), ('img_w', ctypes.c_float), ('wh_ratio_clip', ctypes.c_float),
                ('nms_pre', ctypes.c_int32), ('nms_post', ctypes.c_int32), ('max_num', ctypes.c_int32),
                ('nms_thr', ctypes.c_float),
                ('proposals', ctypes.c_void_p), ('counts', ctypes.c_void_p),
                ('cls_pitch', ctypes.c_int32), ('reg_pitch', ctypes.c_int32)]


class GaRpnDesc(ctypes.Structure):           # hvr_ga_rpn_desc
    _fields_ = [('cls', ctypes.c_void_p), ('reg', ctypes.c_void_p), ('shape', ctypes.c_void_p), ('keep', ctypes.c_void_p),
                ('T', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('anchor_stride', ctypes.c_int32),
                ('cls_pitch', ctypes.c_int32), ('reg_pitch', ctypes.c_int32), ('shape_pitch', ctypes.c_int32),
                ('base_square', ctypes.c_void_p), ('anchoring_means', ctypes.c_void_p), ('anchoring_stds', ctypes.c_void_p),
                ('target_means', ctypes.c_void_p), ('target_stds', ctypes.c_void_p),
                ('img_h', ctypes.c_float), ('img_w', ctypes.c_float), ('wh_ratio_clip', ctypes.c_float),
                ('nms_pre', ctypes.c_int32), ('nms_post', ctypes.c_int32), ('max_num', ctypes.c_int32),
                ('nms_thr', ctypes.c_float),
                ('proposals', ctypes.c_void_p), ('counts', ctypes.c_void_p)]


FPN_MAX_LEVELS = 4   # HVR_FPN_MAX_LEVELS


class RoiLevelsDesc(ctypes.Structure):       # hvr_roi_levels_desc
    _fields_ = [('feat', ctypes.c_void_p * FPN_MAX_LEVELS), ('H', ctypes.c_int32 * FPN_MAX_LEVELS), ('W', ctypes.c_int32 * FPN_MAX_LEVELS),
                ('spatial_scale', ctypes.c_float * FPN_MAX_LEVELS),
                ('L', ctypes.c_int32), ('B', ctypes.c_int32), ('C', ctypes.c_int32), ('K', ctypes.c_int32), ('PH', ctypes.c_int32),
                ('PW', ctypes.c_int32), ('sample_num', ctypes.c_int32), ('dtype', ctypes.c_int32),
                ('finest_scale', ctypes.c_float),
                ('rois', ctypes.c_void_p), ('pool_rois', ctypes.c_void_p), ('out', ctypes.c_void_p), ('levels', ctypes.c_void_p)]


# every symbol include/hvr_hip.h declares: name -> (restype, argtypes)
_vp, _i, _f, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_size_t
SYMBOLS = {
    'hvr_abi_version': (_i, []),
    'hvr_last_error': (ctypes.c_char_p, []),
    'hvr_gemm': (_i, [ctypes.POINTER(GemmDesc), _vp]),
    'hvr_gemm_fewrow_workspace_bytes': (_sz, [ctypes.POINTER(GemmDesc)]),
    'hvr_gemm_splitk_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'hvr_gemm_splitk': (_i, [ctypes.POINTER(GemmDesc), _vp, _sz, _vp]),
    'hvr_gemm_splitk_batched_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'hvr_gemm_splitk_batched': (_i, [ctypes.POINTER(GemmDesc), _i, _i64, _i64, _i64, _vp, _sz, _vp]),
    'hvr_conv2d_nhwc': (_i, [ctypes.POINTER(ConvDesc), _vp]),
    'hvr_conv2d_path': (_i, [ctypes.POINTER(ConvDesc)]),
    'hvr_conv2d_splitk_workspace_bytes': (_sz, [ctypes.POINTER(ConvDesc)]),
    'hvr_conv3x3_grouped': (_i, [ctypes.POINTER(GConvDesc), _vp]),
    'hvr_conv3x3_grouped_supported': (_i, [ctypes.POINTER(GConvDesc)]),
    'hvr_res2_conv3x3': (_i, [ctypes.POINTER(Res2ConvDesc), _vp]),
    'hvr_res2_conv3x3_supported': (_i, [ctypes.POINTER(Res2ConvDesc)]),
    'hvr_avgpool_nhwc': (_i, [ctypes.POINTER(PoolDesc), _vp]),
    'hvr_stem3x3s2_first': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_bottleneck_tail': (_i, [ctypes.POINTER(TailDesc), _vp]),
    'hvr_bottleneck_tail_supported': (_i, [ctypes.POINTER(TailDesc)]),
    'hvr_bottleneck_tail_next': (_i, [ctypes.POINTER(TailNextDesc), _vp]),
    'hvr_bottleneck_tail_next_supported': (_i, [ctypes.POINTER(TailNextDesc)]),
    'hvr_bottleneck_tail_next_live': (_i, [ctypes.POINTER(TailNextLiveDesc), _vp]),
    'hvr_bottleneck_tail_next_live_supported': (_i, [ctypes.POINTER(TailNextLiveDesc)]),
    'hvr_bottleneck_close_sampled': (_i, [ctypes.POINTER(CloseSampledDesc), _vp]),
    'hvr_bottleneck_close_sampled_supported': (_i, [ctypes.POINTER(CloseSampledDesc)]),
    'hvr_im2col_stem': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_maxpool3x3s2_nhwc': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_stem_fused': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'hvr_stem_fused_dtype': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'hvr_relation_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'hvr_relation_fwd': (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp]),
    'hvr_relation_grouped_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'hvr_relation_fwd_grouped': (_i, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _sz, _vp]),
    'hvr_relation_probs_workspace_bytes': (_sz, [_i, _i]),
    'hvr_relation_probs': (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp]),
    'hvr_relation_dscore': (_i, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i, _i64, _i, _f, _i, _vp]),
    'hvr_relu_bwd': (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    'hvr_im2col_nhwc': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'hvr_im2col_t': (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'hvr_relu_bwd_t': (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    'hvr_scale_rows': (_i, [_vp, _vp, _vp, _i, _i64, _i, _vp]),
    'hvr_sgd_workspace_bytes': (_sz, []),
    'hvr_sgd_step': (_i, [_vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _vp, _sz, _i, _vp]),
    'hvr_colsum_workspace_bytes': (_sz, [_i, _i]),
    'hvr_colsum': (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _sz, _vp]),
    'hvr_pack_conv_weight': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_pack_conv_weights_multi': (_i, [_vp, _i, _i64, _i, _vp]),
    'hvr_transpose_multi': (_i, [_vp, _i, _i, _vp]),
    'hvr_unpack_conv_wgrad': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_unpack_conv_wgrads_multi': (_i, [_vp, _i, _i64, _i, _vp]),
    'hvr_det_loss': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp]),
    'hvr_det_loss_sampled': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp]),
    'hvr_max_iou_assign_workspace_bytes': (_sz, [_i, _i]),
    'hvr_max_iou_assign': (_i, [_vp, _i, _i, _vp, _i, _vp, _f, _f, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    'hvr_sample_pos_neg': (_i, [_vp, _vp, _i, _i, _i, ctypes.c_double, _vp, _vp, _vp]),
    'hvr_box_targets': (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    'hvr_rpn_loss': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    'hvr_ce_rows': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    'hvr_sigmoid_focal_loss_fwd': (_i, [_vp, _i, _vp, _i, _i, _f, _f, _i, _vp, _vp]),
    'hvr_sigmoid_focal_loss_bwd': (_i, [_vp, _i, _vp, _vp, _i, _i, _f, _f, _i, _vp, _vp]),
    'hvr_focal_loss_splits': (_i, [_i, _i]),
    'hvr_focal_loss_workspace_bytes': (_sz, [_i, _i]),
    'hvr_focal_loss': (_i, [_vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _sz, _vp, _vp, _vp]),
    'hvr_rpn_focal_loss': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, _vp, _vp]),
    'hvr_reg_loss_fwd': (_i, [_i, _vp, _i, _vp, _i, _i, _f, _f, _f, _vp, _vp]),
    'hvr_reg_loss_bwd': (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp]),
    'hvr_reg_loss_splits': (_i, [_i, _i]),
    'hvr_reg_loss_workspace_bytes': (_sz, [_i, _i]),
    'hvr_reg_loss': (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _f, _f, _vp, _vp, _sz, _vp, _vp, _vp]),
    'hvr_box_loss_fwd': (_i, [_i, _vp, _vp, _i, _f, _f, _vp, _vp]),
    'hvr_box_loss_bwd': (_i, [_i, _vp, _vp, _vp, _i, _f, _f, _vp, _vp]),
    'hvr_box_loss_splits': (_i, [_i]),
    'hvr_box_loss_workspace_bytes': (_sz, [_i]),
    'hvr_box_loss': (_i, [_i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _sz, _vp, _vp, _vp]),
    'hvr_ghm_splits': (_i, [_i, _i]),
    'hvr_ghm_workspace_bytes': (_sz, [_i, _i]),
    'hvr_ghmc_loss': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _f, _vp, _f, _vp, _sz, _vp, _vp, _vp]),
    'hvr_ghmr_loss': (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _i, _f, _vp, _f, _vp, _sz, _vp, _vp, _vp]),
    'hvr_triplet_margin': (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i, _f, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    'hvr_ingest_frame': (_i, [_vp, _i, _i, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    'hvr_ingest_frame_flip': (_i, [_vp, _i, _i, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    'hvr_merge_aug_proposals_workspace_bytes': (_sz, [_i, _i, _i]),
    'hvr_merge_aug_proposals': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    'hvr_map_aug_rois': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'hvr_merge_aug_dets': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'hvr_mining_argreduce': (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp]),
    'hvr_roi_align_fwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp]),
    'hvr_roi_align_bwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    'hvr_deform_im2col_supported': (_i, [_i, _i, _i]),
    'hvr_deform_im2col': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _i, _vp]),
    'hvr_deform_roi_pool_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _i64, _i64, _i, _vp]),
    'hvr_roi_pool_fwd': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    'hvr_roi_pool_bwd': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'hvr_fpn_merge_supported': (_i, [_i, _i, _i]),
    'hvr_fpn_merge': (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    'hvr_roi_align_levels_supported': (_i, [_i, _i, _i]),
    'hvr_roi_align_levels_fwd': (_i, [ctypes.POINTER(RoiLevelsDesc), _vp]),
    'hvr_gcb_supported': (_i, [_i, _i]),
    'hvr_gcb_splits': (_i, [_i, _i, _i]),
    'hvr_gcb_workspace_bytes': (_sz, [_i, _i, _i]),
    'hvr_gcb_pool': (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _vp]),
    'hvr_gcb_transform': (_i, [_vp, _sz, _i, _i, _i, _i, ctypes.POINTER(GcbMlp), ctypes.POINTER(GcbMlp), _vp, _vp, _vp]),
    'hvr_gcb_apply': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'hvr_gn_supported': (_i, [_i, _i, _i]),
    'hvr_gn_splits': (_i, [_i, _i, _i]),
    'hvr_gn_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'hvr_gn_stats': (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    'hvr_gn_apply': (_i, [_vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'hvr_gen_attn_supported': (_i, [_i, _i, _i, _i, _i]),
    'hvr_gen_attn_query_tile': (_i, []),
    'hvr_gen_attn_key_block': (_i, []),
    'hvr_gen_attn_fwd': (_i, [ctypes.POINTER(GenAttnDesc), _vp]),
    'hvr_nms_workspace_bytes': (_sz, [_i]),
    'hvr_nms_first': (_i, [_vp, _i, _f, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    'hvr_nms': (_i, [_vp, _i, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    'hvr_rpn_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'hvr_rpn_proposals': (_i, [ctypes.POINTER(RpnDesc), _vp, _sz, _vp]),
    'hvr_rpn_wide_frames': (_i, [_i]),
    'hvr_ga_mask_offsets': (_i, [_vp, _i64, _f, _vp, _vp, _i64, _vp, _vp, _i64, _i, _i64, _vp]),
    'hvr_masked_conv_max_cout': (_i, []),
    'hvr_masked_conv_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _i, _vp]),
    'hvr_ga_rpn_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'hvr_ga_rpn_proposals': (_i, [ctypes.POINTER(GaRpnDesc), _vp, _sz, _vp]),
    'hvr_det_decode': (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _f, _f, _f, _f, _vp, _vp, _vp]),
    'hvr_multiclass_nms_workspace_bytes': (_sz, [_i, _i]),
    'hvr_multiclass_nms': (_i, [_vp, _vp, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'hvr_soft_nms_workspace_bytes': (_sz, [_i]),
    'hvr_soft_nms': (_i, [_vp, _i, _f, _i, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    'hvr_multiclass_soft_nms_workspace_bytes': (_sz, [_i, _i, _i]),
    'hvr_multiclass_soft_nms': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'hvr_seq_nms_workspace_bytes': (_sz, [_i, _i, _i]),
    'hvr_seq_nms': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'hvr_seq_nms_phases': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    'hvr_seq_nms_batched_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'hvr_seq_nms_batched': (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    'hvr_cast': (_i, [_vp, _vp, _i64, _i, _i, _vp]),
    'hvr_cast_scaled': (_i, [_vp, _vp, _i64, _i, _i, _f, _vp]),
    'hvr_permute_nchw_nhwc': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'hvr_transpose_pad': (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _vp]),
}

_lib = None


def build(force=False):
    """Compile the HIP sources for gfx950 into ``hvrnet_amd/libhvr_hip.so`` (in-tree)."""
    script = os.path.join(_HERE, 'csrc', 'build.sh')
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
        for f in os.listdir(os.path.join(_HERE, 'csrc', 'build')) if os.path.isdir(os.path.join(_HERE, 'csrc', 'build')) else []:
            os.remove(os.path.join(_HERE, 'csrc', 'build', f))
    subprocess.run(['bash', script], check=True)
    return LIB_PATH


def lib():
    """The loaded library; raises HvrError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HvrError('libhvr_hip.so is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(there is no CPU or PyTorch fallback for the HVR hot path)')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.hvr_abi_version() != ABI_VERSION:
            raise HvrError('libhvr_hip.so has ABI version %d, this binding needs %d: rebuild it (hvrnet_amd/csrc/build.sh)'
                           % (handle.hvr_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def _check(rc, what):
    if rc != 0:
        raise HvrError('%s failed (%d): %s' % (what, rc, lib().hvr_last_error().decode()))


def _raw_stream(device=None):
    """hipStream_t of torch's current stream as an int.  torch.cuda.current_stream() builds a Stream object (and re-checks
    availability) on every call, ~3-9 us; a training iteration asks ~1 700 times, so go to the raw getter."""
    idx = torch._C._cuda_getDevice() if device is None or device.index is None else device.index
    return torch._C._cuda_getCurrentRawStream(idx)


def _stream():
    return ctypes.c_void_p(_raw_stream())


DTYPE_CODES = {torch.float32: HVR_F32, torch.bfloat16: HVR_BF16, torch.float16: HVR_F16, SPLIT: HVR_F16S}


def _dt(t):
    if t.dtype not in DTYPE_CODES:
        raise HvrError('unsupported tensor dtype %s (float32 / bfloat16 / float16 / the split-half container int32)' % t.dtype)
    return DTYPE_CODES[t.dtype]


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise NotImplementedError('hvr_hip ops run on the GPU only; got a %s tensor' % t.device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _out(out, shape, dtype, device):
    """The `out=` contract of the wrappers (the caller-allocates contract of the C ABI): `out` when given -- a contiguous tensor of exactly
    this shape, dtype and device, e.g. a slice of a larger batch -- else a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous() and out.device == device, \
        (tuple(out.shape), tuple(shape), out.dtype, dtype)
    return out


# ---- optional per-call timing with HIP events on the launch stream (used by bench.py) ----
_prof = None


class _Span(object):
    __slots__ = ('tag', 'work', 'start')

    def __init__(self, tag, work):
        self.tag, self.work = tag, work

    def __enter__(self):
        self.start = torch.cuda.Event(enable_timing=True)
        self.start.record(torch.cuda.current_stream())

    def __exit__(self, *exc):
        end = torch.cuda.Event(enable_timing=True)
        end.record(torch.cuda.current_stream())
        _prof['spans'].append((self.tag, self.work, self.start, end))


class _NoSpan(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NOSPAN = _NoSpan()


def _span(tag, work=0.0):
    if _prof is None or (tag.split(' ')[0] not in _prof['tags'] and '*' not in _prof['tags']):
        return _NOSPAN
    return _Span(tag, work)


def profile_begin(tags=('*',), detail=False):
    """Start recording (tag, algorithmic work, HIP-event pair) for the C-ABI calls whose tag is in `tags`."""
    global _prof
    _prof = dict(tags=set(tags), spans=[], detail=detail)


def profile_end(raw=False):
    """-> {tag: dict(calls, ms, work)}; synchronises once.  raw: the calls in issue order, [(tag, work, ms)]."""
    global _prof
    spans, _prof = _prof['spans'], None
    torch.cuda.synchronize()
    if raw:
        return [(tag, work, s.elapsed_time(e)) for tag, work, s, e in spans]
    out = {}
    for tag, work, s, e in spans:
        d = out.setdefault(tag, dict(calls=0, ms=0.0, work=0.0))
        d['calls'] += 1
        d['ms'] += s.elapsed_time(e)
        d['work'] += work
    return out


_zero_pages = {}


def zero_page(device):
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.uint8, device=device)
        torch.cuda.current_stream(device).synchronize()  # once per device: every stream reads this page afterwards
        _zero_pages[device] = z
    return z


def kstep(dtype):
    return 32 if dtype == torch.float32 else 64


# A split-half value below 2^-3 keeps an absolute, not a relative, error bound (its lo half is then a half subnormal), so this
# layer keeps split tensors SCALED by powers of two: weights x 2^6 (they are ~1e-2), activations x 2^4 (full precision from
# 2^-7 up, range 4094).  cast() applies / removes the activation scale, as_operand() the weight scale, and gemm() / conv2d_nhwc()
# hand the kernels the factors that keep every output in its convention: alpha on the accumulators, beta on the bias.  Every B
# operand those two are given here is a weight matrix made by as_operand().  Nothing outside this file knows about the scales.
SPLIT_WEIGHT_SCALE = 64.0
SPLIT_ACT_SCALE = 16.0


def _split_factors(out_is_f32, alpha):
    """(alpha, beta) of a split-half product A(x ACT) . W(x WEIGHT)^T whose output is a scaled split tensor or true-valued f32."""
    if alpha is not None:
        return float(alpha), 1.0
    if out_is_f32:
        return 1.0 / (SPLIT_WEIGHT_SCALE * SPLIT_ACT_SCALE), 1.0
    return 1.0 / SPLIT_WEIGHT_SCALE, SPLIT_ACT_SCALE


def as_operand(t, dtype):
    """An f32 WEIGHT tensor (pack time) in the operand format `dtype`, contiguous (split half: x SPLIT_WEIGHT_SCALE)."""
    t = t.contiguous()
    if dtype == SPLIT:
        return cast(t.float(), SPLIT, scale=SPLIT_WEIGHT_SCALE)
    return t.to(dtype)


# ----------------------------------------------------------------------------------------
def gemm(a, w, bias=None, resid=None, relu=False, out_f32=False, out=None, staging=None, tile=None, alpha=None):
    """out[M,N] = act(a[M,K] @ w[N,K]^T + bias + resid).  a / w / resid share one dtype.  alpha (split half only): the factor on
    the accumulators (bias then unscaled); default: the factors of this layer's scaled split tensors (_split_factors)."""
    _need_cuda(a, w, bias, resid)
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], (a.shape, w.shape)
    assert a.stride(1) == 1 and w.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32 if out_f32 else a.dtype, device=a.device)
    d = GemmDesc(A=a.data_ptr(), B=w.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K,
                 lda=a.stride(0), ldb=w.stride(0), ldc=out.stride(0),
                 bias=bias.data_ptr() if bias is not None else None,
                 resid=resid.data_ptr() if resid is not None else None,
                 ldr=resid.stride(0) if resid is not None else 0,
                 relu=int(relu), out_f32=int(out.dtype == torch.float32 and a.dtype != torch.float32),
                 dtype=_dt(a), staging=STAGING if staging is None else staging,
                 tile_hint=TILE_HINT if tile is None else tile)
    if a.dtype == SPLIT:
        if resid is not None and out.dtype == torch.float32:
            # a split residual is stored x SPLIT_ACT_SCALE and the epilogue adds it as it is: right for a scaled split output, 16 x
            # too much beside a true-valued f32 one
            raise HvrError('split-half gemm: a residual cannot be combined with an f32 output (the residual carries the activation scale)')
        d.alpha, d.beta = _split_factors(out.dtype == torch.float32, alpha)
    nbytes = lib().hvr_gemm_fewrow_workspace_bytes(ctypes.byref(d)) if _fewrow[0] else 0   # few rows, long K: K slices + one reduce launch
    if nbytes:
        ws = _workspace(nbytes, a.device, 'gemm_fewrow')
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    with _span('gemm' if not (_prof and _prof['detail']) else 'gemm M%d N%d K%d' % (M, N, K), 2.0 * M * N * K):
        _check(lib().hvr_gemm(ctypes.byref(d), _stream()), 'hvr_gemm')
    return out


def gemm_splitk(a, w, staging=None, tile=None, out=None):
    """f32 out[M,N] = a[M,K] @ w[N,K]^T for few-tile / long-K products (weight gradients): K slices in one launch + a reduce.
    out: a contiguous f32 [M, N] tensor to write into (e.g. a parameter's gradient buffer) instead of a fresh one."""
    _need_cuda(a, w)
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.dtype == w.dtype, (a.shape, w.shape)
    assert a.stride(1) == 1 and w.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    out = _out(out, (M, N), torch.float32, a.device)
    d = GemmDesc(A=a.data_ptr(), B=w.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K, lda=a.stride(0), ldb=w.stride(0), ldc=N,
                 bias=None, resid=None, ldr=0, relu=0, out_f32=int(a.dtype != torch.float32), dtype=_dt(a),
                 staging=STAGING if staging is None else staging, tile_hint=TILE_HINT if tile is None else tile)
    nbytes = lib().hvr_gemm_splitk_workspace_bytes(M, N, K, _dt(a))
    ws = _workspace(nbytes, a.device, 'splitk') if nbytes else None
    with _span('gemm' if not (_prof and _prof['detail']) else 'gemm M%d N%d K%d splitk' % (M, N, K), 2.0 * M * N * K):
        _check(lib().hvr_gemm_splitk(ctypes.byref(d), _ptr(ws), nbytes, _stream()), 'hvr_gemm_splitk')
    return out


def gemm_splitk_batched(a, w, out=None):
    """f32 out[g] = a[g] @ w[g]^T for g < G: a [G, M, K], w [G, N, K] (leading slices of contiguous slabs), one launch (+ one reduce
    when K is cut into slices) for the G weight gradients of a stage's identical blocks.  -> out [G, M, N] f32."""
    _need_cuda(a, w)
    assert a.dim() == 3 and w.dim() == 3 and a.shape[0] == w.shape[0] and a.shape[2] == w.shape[2] and a.dtype == w.dtype
    assert a.stride(2) == 1 and w.stride(2) == 1 and a.stride(1) == a.shape[2] and w.stride(1) == w.shape[2]
    G, M, K = a.shape
    N = w.shape[1]
    out = _out(out, (G, M, N), torch.float32, a.device)
    d = GemmDesc(A=a.data_ptr(), B=w.data_ptr(), C=out.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=None, resid=None, ldr=0, relu=0,
                 out_f32=int(a.dtype != torch.float32), dtype=_dt(a), staging=STAGING, tile_hint=TILE_HINT)
    nbytes = lib().hvr_gemm_splitk_batched_workspace_bytes(M, N, K, _dt(a), G)
    ws = _workspace(nbytes, a.device, 'splitk_batched') if nbytes else None
    with _span('gemm' if not (_prof and _prof['detail']) else 'gemm %dx M%d N%d K%d splitk batched' % (G, M, N, K), 2.0 * G * M * N * K):
        _check(lib().hvr_gemm_splitk_batched(ctypes.byref(d), G, a.stride(0), w.stride(0), M * N, _ptr(ws), nbytes, _stream()), 'hvr_gemm_splitk_batched')
    return out


def conv2d_nhwc(x, w, bias=None, resid=None, relu=False, stride=1, pad=0, dil=1, out_f32=False, staging=None, tile=None, out=None, alpha=None):
    """x [B,H,W,Cin] (physical NHWC), w [Cout,KH,KW,Cin] -> [B,OH,OW,Cout]; out: a contiguous tensor of that shape and the
    output dtype to write into (the caller-allocates contract of the C ABI) instead of a fresh one."""
    _need_cuda(x, w, bias, resid)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    y = _out(out, (B, OH, OW, Cout), torch.float32 if out_f32 else x.dtype, x.device)
    d = ConvDesc(x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW,
                 stride=stride, pad=pad, dil=dil,
                 bias=bias.data_ptr() if bias is not None else None,
                 resid=resid.data_ptr() if resid is not None else None,
                 relu=int(relu), out_f32=int(out_f32 and x.dtype != torch.float32), dtype=_dt(x),
                 staging=STAGING if staging is None else staging, tile_hint=TILE_HINT if tile is None else tile,
                 zero=zero_page(x.device).data_ptr())
    if x.dtype == SPLIT:
        if resid is not None and out_f32:
            raise HvrError('split-half conv: a residual cannot be combined with an f32 output (the residual carries the activation scale)')
        d.alpha, d.beta = _split_factors(bool(out_f32), alpha)
    # few-row problems (one frame through the stride-16 stages): the library cuts the K loop into slices when it is handed
    # scratch for the f32 partial tiles (per stream, like every other workspace here)
    nbytes = lib().hvr_conv2d_splitk_workspace_bytes(ctypes.byref(d)) if _fewrow[0] else 0
    if nbytes:
        ws = _workspace(nbytes, x.device, 'conv_splitk')
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    tag, work = 'conv', 2.0 * B * OH * OW * Cout * KH * KW * Cin
    if _prof is not None and ('*' in _prof['tags'] or 'conv' in _prof['tags'] or 'conv_expand' in _prof['tags']):
        if lib().hvr_conv2d_path(ctypes.byref(d)) == 1:
            # the HBM-bound expand + residual convs (expand.hip) are accounted in bytes: X, residual and output once, W once
            tag, work = 'conv_expand', float((B * OH * OW * (Cin + (2 if resid is not None else 1) * Cout) + Cout * Cin) * x.element_size())
        if _prof['detail']:
            tag = '%s %dx%d %d->%d k%d s%d d%d%s' % (tag, H, W, Cin, Cout, KH, stride, dil, '+res' if resid is not None else '')
    with _span(tag, work):
        _check(lib().hvr_conv2d_nhwc(ctypes.byref(d), _stream()), 'hvr_conv2d_nhwc')
    return y


# ---- the fused Bottleneck entries.  Each descriptor is built once, by shape, with placeholder addresses: a query by shape (*_path) hands
# it to the library as it is -- nothing is launched, no memory is touched -- and the launch points it at its tensors first.
_PH = 1 << 20   # the placeholder address: 128-byte aligned, as every map the torch allocator or backbone.as_nhwc hands out


def _launch_fused(entry, d, nbytes, detail, args):
    """Launches `entry` on descriptor d inside a 'conv_expand' span (the HBM-bound row-panel family, accounted in the bytes it moves)."""
    tag = 'conv_expand ' + detail % args if _prof is not None and _prof['detail'] else 'conv_expand'
    with _span(tag, float(nbytes)):
        _check(getattr(lib(), entry)(ctypes.byref(d), _stream()), entry)


def _point(d, **tensors):
    """Descriptor d with the address of every tensor given (None: the field stays as the shape form left it)."""
    for field, t in tensors.items():
        if t is not None:
            setattr(d, field, t.data_ptr())
    return d


def _tail_form(code, B, OH, OW, C1, Cout, x_hwc=None, stride2=1, relu=True):
    """x_hwc: (H2, W2, C2) of the input map a projection block samples at stride2 as its second K segment; None: no second segment."""
    H2, W2, C2 = x_hwc if x_hwc is not None else (OH, OW, 0)
    return TailDesc(h=_PH, x=_PH if x_hwc is not None else None, w=_PH, y=_PH, B=B, OH=OH, OW=OW, C1=C1, H2=H2, W2=W2, C2=C2,
                    stride2=int(stride2) if x_hwc is not None else 1, Cout=Cout, bias=_PH, relu=int(relu), dtype=code)


def _tail_desc(h, x, w, bias, stride2, relu, y):
    B, OH, OW, C1 = h.shape
    return _point(_tail_form(_dt(h), B, OH, OW, C1, w.shape[0], tuple(x.shape[1:]), stride2, relu), h=h, x=x, w=w, bias=bias, y=y)


def tail_path(B, OH, OW, C1, Cout, x_hwc, stride2=1, dtype=torch.bfloat16):
    """Whether hvr_bottleneck_tail has a fused kernel for a projection block of these shapes (bf16 / half, C1 + C2 in {128, 384}, ...)."""
    return bool(lib().hvr_bottleneck_tail_supported(ctypes.byref(_tail_form(DTYPE_CODES.get(dtype, HVR_F32), B, OH, OW, C1, Cout, x_hwc, stride2))))


def bottleneck_tail_supported(h, x, w, bias, stride2):
    """tail_path for these tensors (on the device, bf16 / half, one dtype, contiguous)."""
    if not (h.is_cuda and h.dtype in (torch.bfloat16, torch.float16) and x.dtype == h.dtype and h.is_contiguous() and x.is_contiguous()):
        return False
    return tail_path(h.shape[0], h.shape[1], h.shape[2], h.shape[3], w.shape[0], tuple(x.shape[1:]), stride2, h.dtype)


def bottleneck_tail(h, x, w, bias, stride2=1, relu=True, out=None):
    """relu(h W3^T + x_s Wd^T + bias): the closing 1x1 of a Bottleneck with its projection shortcut as a second K segment.
    h [B,OH,OW,C1], x [B,H2,W2,C2] physical NHWC, w [Cout, C1 + C2], bias f32 [Cout] -> [B,OH,OW,Cout]."""
    _need_cuda(h, x, w, bias)
    B, OH, OW, C1 = h.shape
    Cout = w.shape[0]
    y = _out(out, (B, OH, OW, Cout), h.dtype, h.device)
    d = _tail_desc(h, x, w, bias, stride2, relu, y)
    _launch_fused('hvr_bottleneck_tail', d, (h.numel() + B * OH * OW * x.shape[3] + y.numel() + w.numel()) * h.element_size(),
                  'tail %dx%d %d+%d->%d s%d', (OH, OW, C1, x.shape[3], Cout, stride2))
    return y


def _tail_next_form(code, B, OH, OW, C1, Cout, Cn, x_hwc=None, stride2=1):
    """x_hwc as _tail_form: given for a projection block (its input map is the second K segment), None for an identity block (a residual map)."""
    d = TailNextDesc(tail=_tail_form(code, B, OH, OW, C1, Cout, x_hwc, stride2), resid=_PH if x_hwc is None else None, wn=_PH, bias_n=_PH,
                     hn=_PH, Cn=Cn)
    if code == HVR_F16S:   # both products: scaled split activations x scaled split weights -> a scaled split activation
        d.alpha, d.beta = _split_factors(False, None)
    return d


def _tail_next_desc(h, x, resid, w, bias, stride2, wn, bias_n, y, hn):
    B, OH, OW, C1 = h.shape
    d = _tail_next_form(_dt(h), B, OH, OW, C1, w.shape[0], wn.shape[0], tuple(x.shape[1:]) if x is not None else None, stride2)
    _point(d.tail, h=h, x=x, w=w, bias=bias, y=y)
    d.resid = resid.data_ptr() if resid is not None else None
    return _point(d, wn=wn, bias_n=bias_n, hn=hn)


def tail_next_path(B, OH, OW, C1, Cout, Cn, x_hwc=None, stride2=1, dtype=torch.bfloat16):
    """Whether hvr_bottleneck_tail_next runs these shapes: (Cout, Cn) = (256, 64) / (512, 128) in bf16 / half, the projection form (x_hwc) or the
    identity form; split half: the identity form with (Cout, Cn) = (256, 64)."""
    return bool(lib().hvr_bottleneck_tail_next_supported(ctypes.byref(
        _tail_next_form(DTYPE_CODES.get(dtype, HVR_F32), B, OH, OW, C1, Cout, Cn, x_hwc, stride2))))


def bottleneck_tail_next_supported(h, x, resid, w, bias, stride2, wn, bias_n):
    """tail_next_path for these tensors (on the device, bf16 / half / split half, one dtype, contiguous, exactly one of x and resid)."""
    ts = [t for t in (h, x, resid) if t is not None]
    if not all(t.is_cuda and t.dtype in FUSED_DTYPES and t.dtype == h.dtype and t.is_contiguous() for t in ts):
        return False
    if h.dtype == SPLIT and (x is not None or wn.dtype != SPLIT or w.dtype != SPLIT):
        return False
    if (x is None) == (resid is None) or wn.dim() != 2 or wn.shape[1] != w.shape[0] or not wn.is_contiguous():
        return False
    return tail_next_path(h.shape[0], h.shape[1], h.shape[2], h.shape[3], w.shape[0], wn.shape[0], tuple(x.shape[1:]) if x is not None else None,
                          stride2, h.dtype)


def bottleneck_tail_next(h, x, resid, w, bias, wn, bias_n, stride2=1, out=None):
    """y = relu(h W3^T [+ x_s Wd^T] + bias [+ resid]) and hn = relu(y wn^T + bias_n), the next block's conv1, in one pass.
    Exactly one of x (projection block: its input map) and resid (identity block) is given.  -> (y, hn)"""
    _need_cuda(h, w, bias, wn, bias_n)
    B, OH, OW, C1 = h.shape
    Cout, Cn = w.shape[0], wn.shape[0]
    y = _out(out, (B, OH, OW, Cout), h.dtype, h.device)
    hn = torch.empty((B, OH, OW, Cn), dtype=h.dtype, device=h.device)
    d = _tail_next_desc(h, x, resid, w, bias, stride2, wn, bias_n, y, hn)
    side = x if x is not None else resid
    _launch_fused('hvr_bottleneck_tail_next', d,
                  (h.numel() + B * OH * OW * side.shape[3] + y.numel() + hn.numel() + w.numel() + wn.numel()) * h.element_size(),
                  'tail+next %dx%d %d+%d->%d->%d', (OH, OW, C1, x.shape[3] if x is not None else 0, Cout, Cn))
    return y, hn


def _tail_next_live_desc(h, resid, w, bias, wn, bias_n, live_stride, y, hn):
    return TailNextLiveDesc(next=_tail_next_desc(h, None, resid, w, bias, 1, wn, bias_n, y, hn), live_stride=int(live_stride))


def bottleneck_tail_next_live_supported(h, resid, w, bias, wn, bias_n, live_stride=2):
    """True when hvr_bottleneck_tail_next_live runs these shapes: an identity block, (Cout, Cn, C1) = (256, 64, 64) / (512, 128, 128) in
    bf16 / half, (256, 64, 64) in split half, contiguous maps, at least 128 pixels."""
    if not all(t.is_cuda and t.dtype in FUSED_DTYPES and t.dtype == h.dtype and t.is_contiguous() for t in (h, resid, w, wn)):
        return False
    if h.dim() != 4 or resid.dim() != 4 or wn.dim() != 2 or w.dim() != 2 or wn.shape[1] != w.shape[0] or int(live_stride) < 1:
        return False
    if tuple(resid.shape) != tuple(h.shape[:3]) + (w.shape[0],) or w.shape[1] != h.shape[3]:
        return False
    return tail_next_live_path(h.shape[0], h.shape[1], h.shape[2], h.shape[3], w.shape[0], wn.shape[0], live_stride, h.dtype)


def tail_next_live_path(B, OH, OW, C1, Cout, Cn, live_stride=2, dtype=torch.bfloat16):
    """Whether hvr_bottleneck_tail_next_live has a kernel for an identity block of these shapes (the query by shape: nothing is launched)."""
    d = TailNextLiveDesc(next=_tail_next_form(DTYPE_CODES.get(dtype, HVR_F32), B, OH, OW, C1, Cout, Cn), live_stride=int(live_stride))
    return bool(lib().hvr_bottleneck_tail_next_live_supported(ctypes.byref(d)))


def bottleneck_tail_next_live(h, resid, w3, b3, wn, bn, live_stride=2, out=None, out_hn=None):
    """bottleneck_tail_next's identity form for a block whose output only a stride-`live_stride` consumer reads besides the next block's
    conv1: y = relu(h W3^T + b3 + resid) is computed everywhere and written at pixels (s oy, s ox) only, as the compact map
    y_live [B,(OH-1)//s+1,(OW-1)//s+1,Cout] = bottleneck_tail_next(...)[0][:, ::s, ::s] bit for bit; hn = relu(y wn^T + bn) [B,OH,OW,Cn]
    at full resolution, bit for bit as well.  The dead pixels are computed and not stored (their lanes are masked out of the stores), so
    there is no scratch and nothing to allocate inside a captured region but the two outputs.  -> (y_live, hn)"""
    _need_cuda(h, resid, w3, b3, wn, bn)
    B, OH, OW, C1 = h.shape
    Cout, Cn, s = w3.shape[0], wn.shape[0], int(live_stride)
    LH, LW = (OH - 1) // s + 1, (OW - 1) // s + 1
    assert h.is_contiguous() and resid.is_contiguous() and tuple(resid.shape) == (B, OH, OW, Cout) and resid.dtype == h.dtype
    y, hn = _out(out, (B, LH, LW, Cout), h.dtype, h.device), _out(out_hn, (B, OH, OW, Cn), h.dtype, h.device)
    d = _tail_next_live_desc(h, resid, w3, b3, wn, bn, s, y, hn)
    # bytes it moves: h, the residual and hn at every pixel, y at the live ones, W3 and Wn once
    _launch_fused('hvr_bottleneck_tail_next_live', d, (h.numel() + resid.numel() + y.numel() + hn.numel() + w3.numel() + wn.numel()) * h.element_size(),
                  'tail+next live/%d %dx%d %d+0->%d->%d', (s, OH, OW, C1, Cout, Cn))
    return y, hn


def _close_sampled_form(code, B, OH, OW, C1, Cout, RH, RW, stride, relu=True):
    d = CloseSampledDesc(h=_PH, w=_PH, resid=_PH, y=_PH, B=B, OH=OH, OW=OW, C1=C1, Cout=Cout, RH=RH, RW=RW, rstride=int(stride), bias=_PH,
                         relu=int(relu), dtype=code)
    if code == HVR_F16S:
        d.alpha, d.beta = _split_factors(False, None)
    return d


def _close_sampled_desc(h, w, bias, resid, stride, relu, y):
    B, OH, OW, C1 = h.shape
    _, RH, RW, Cout = resid.shape
    return _point(_close_sampled_form(_dt(h), B, OH, OW, C1, Cout, RH, RW, stride, relu), h=h, w=w, bias=bias, resid=resid, y=y)


def bottleneck_close_sampled_supported(h, w, bias, resid, stride):
    """True when hvr_bottleneck_close_sampled runs these shapes: bf16 / half / split half on the row-panel kernels, contiguous maps,
    h [B,OH,OW,C1] compact, resid [B,RH,RW,Cout] at full resolution with (OH - 1) stride < RH and (OW - 1) stride < RW."""
    if not (h.is_cuda and h.dtype in FUSED_DTYPES and resid.dtype == h.dtype and w.dtype == h.dtype
            and h.is_contiguous() and resid.is_contiguous() and w.is_contiguous() and h.dim() == 4 and resid.dim() == 4):
        return False
    if h.shape[0] != resid.shape[0] or w.numel() != resid.shape[3] * h.shape[3] or w.shape[0] != resid.shape[3]:
        return False
    return close_sampled_path(h.shape[0], h.shape[1], h.shape[2], h.shape[3], resid.shape[3], resid.shape[1], resid.shape[2], stride, h.dtype)


def close_sampled_path(B, OH, OW, C1, Cout, RH, RW, stride=2, dtype=torch.bfloat16):
    """Whether hvr_bottleneck_close_sampled has a kernel for these shapes (the query by shape: placeholder addresses, nothing is launched)."""
    return bool(lib().hvr_bottleneck_close_sampled_supported(ctypes.byref(
        _close_sampled_form(DTYPE_CODES.get(dtype, HVR_F32), B, OH, OW, C1, Cout, RH, RW, stride))))


def bottleneck_close_sampled(h, w, bias, resid, stride=2, relu=True, out=None):
    """y[b,oy,ox] = act(h[b,oy,ox] W3^T + bias + resid[b, oy stride, ox stride]): the closing 1x1 of a stage's last block on the pixels
    the next stage's stride-2 1x1 convs read.  h [B,OH,OW,C1] (conv2 run at that stride), resid [B,RH,RW,Cout] the block's
    full-resolution input, w [Cout,C1] (or [Cout,1,1,C1]), bias f32 [Cout] -> [B,OH,OW,Cout]; bit-identical to
    conv2d_nhwc(h_full, w, bias, resid=resid, relu=relu)[:, ::stride, ::stride]."""
    _need_cuda(h, w, bias, resid)
    B, OH, OW, C1 = h.shape
    _, RH, RW, Cout = resid.shape
    assert h.is_contiguous() and resid.is_contiguous() and w.is_contiguous() and resid.dtype == h.dtype and w.dtype == h.dtype
    assert w.shape[0] == Cout and w.numel() == Cout * C1 and resid.shape[0] == B, (tuple(w.shape), tuple(resid.shape))
    y = _out(out, (B, OH, OW, Cout), h.dtype, h.device)
    d = _close_sampled_desc(h, w, bias, resid, stride, relu, y)
    # bytes it moves: h, the sampled residual rows and y once, W once
    _launch_fused('hvr_bottleneck_close_sampled', d, (B * OH * OW * (C1 + 2 * Cout) + Cout * C1) * h.element_size(),
                  'sampled %dx%d<-%dx%d %d->%d k1+res s%d', (OH, OW, RH, RW, C1, Cout, stride))
    return y


def conv2d_path(B, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, dtype=torch.bfloat16, resid=True, bias=True, out_f32=False, tile=0):
    """Which kernel hvr_conv2d_nhwc would run for a conv of this shape (0 tile engine, 1 expand.hip panel kernel, < 0 rejected).
    Nothing is launched and no memory is touched: the descriptor carries placeholder (16-byte aligned) addresses."""
    d = ConvDesc(x=_PH, w=_PH, y=_PH, B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k, stride=stride, pad=pad, dil=dil,
                 bias=_PH if bias else None, resid=_PH if resid else None, relu=1, out_f32=int(out_f32),
                 dtype=DTYPE_CODES.get(dtype, HVR_F32), staging=STAGING, tile_hint=tile, zero=_PH)
    return int(lib().hvr_conv2d_path(ctypes.byref(d)))


def conv3x3_grouped_supported(B, H, W, C, groups, stride=1, dil=1, dtype=torch.bfloat16, pad=None):
    """True where hvr_conv3x3_grouped has an instance for a grouped 3x3 of this shape (gconv3x3.hip: bf16 / half, C / groups in
    {4, 8, 16, 32}, C % 64 == 0 up to 2048, stride 1 / 2, pad == dil in {1, 2}).  Nothing is launched: placeholder addresses."""
    d = GConvDesc(x=_PH, w=_PH, y=_PH, bias=_PH, B=B, H=H, W=W, C=C, groups=groups, stride=stride, pad=dil if pad is None else pad, dil=dil,
                  relu=1, dtype=DTYPE_CODES.get(dtype, -1))
    return bool(lib().hvr_conv3x3_grouped_supported(ctypes.byref(d)))


class GroupedWeight(object):
    """The weight of a grouped 3x3 conv, w [C,3,3,Cg] (f32, or exactly representable in f32), in the operand format `dtype`: the grouped
    form the kernel reads, and the block-diagonal dense form [C,3,3,C] (exact zeros outside the groups) that conv2d_nhwc takes.  Each
    is built on first use (pack time) and kept: a model that never leaves the grouped kernel never holds the dense one."""

    def __init__(self, w, dtype):
        assert w.dim() == 4 and tuple(w.shape[1:3]) == (3, 3) and w.shape[0] % w.shape[3] == 0, tuple(w.shape)
        self.w32, self.dtype = w.detach().float().contiguous(), dtype
        self.C, self.Cg = int(w.shape[0]), int(w.shape[3])
        self.groups = self.C // self.Cg
        self._grouped = self._dense = None

    def grouped(self):
        if self._grouped is None:
            if self.dtype == SPLIT:
                raise HvrError('a split-half grouped weight has no grouped form (rows of %d elements; the container holds groups of 32): '
                               'the dense route carries this mode' % self.Cg)
            self._grouped = self.w32.to(self.dtype)
        return self._grouped

    def dense(self):
        if self._dense is None:
            G, Cg = self.groups, self.Cg
            full = torch.zeros((G, Cg, 3, 3, G, Cg), dtype=torch.float32, device=self.w32.device)
            g = torch.arange(G, device=self.w32.device)
            full[g, :, :, :, g, :] = self.w32.view(G, Cg, 3, 3, Cg)
            self._dense = as_operand(full.view(self.C, 3, 3, self.C), self.dtype)
        return self._dense


def conv3x3_grouped(x, w, bias, relu, stride, dil, out=None, route=None):
    """act(grouped 3x3 conv of x [B,H,W,C] (physical NHWC) + bias) -> [B,OH,OW,C], pad = dil (the rule: include/hvr_hip.h,
    hvr_conv3x3_grouped).  w: a GroupedWeight, or a [C,3,3,Cg] tensor (packed on every call: tests and tools).
    route: None = the grouped kernel where it has an instance for this shape and format, else conv2d_nhwc on the block-diagonal dense
    weight; 'grouped' / 'dense' force one (the forced kernel raises HvrError where it has no instance)."""
    assert route in (None, 'grouped', 'dense'), route
    _need_cuda(x, bias)
    gw = w if isinstance(w, GroupedWeight) else GroupedWeight(w, x.dtype)
    _need_cuda(gw.w32)
    assert gw.dtype == x.dtype, (gw.dtype, x.dtype)
    B, H, W, C = x.shape
    if route is None:
        route = 'grouped' if C == gw.C and conv3x3_grouped_supported(B, H, W, C, gw.groups, stride, dil, x.dtype) else 'dense'
    if route == 'dense':
        return conv2d_nhwc(x, gw.dense(), bias, relu=relu, stride=stride, pad=dil, dil=dil, out=out)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if C != gw.C:
        raise HvrError('hvr_conv3x3_grouped: x has %d channels, the weight %d' % (C, gw.C))
    assert x.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == C
    y = _out(out, (B, OH, OW, C), x.dtype, x.device)
    # (the library checks the shape before it launches anything: a forced route outside the instance set raises here)
    d = _point(GConvDesc(B=B, H=H, W=W, C=C, groups=gw.groups, stride=stride, pad=dil, dil=dil, relu=int(relu), dtype=_dt(x)),
               x=x, w=gw.grouped(), y=y, bias=bias)
    # bytes it moves: the map in and out once, the weights once
    tag = 'gconv' if not (_prof and _prof['detail']) else 'gconv %dx%d %d/%d s%d d%d' % (H, W, C, gw.groups, stride, dil)
    with _span(tag, float((B * H * W * C + B * OH * OW * C + 9 * C * gw.Cg) * x.element_size())):
        _check(lib().hvr_conv3x3_grouped(ctypes.byref(d), _stream()), 'hvr_conv3x3_grouped')
    return y


# ---- Res2Net: the 3x3 conv over a channel slice with a pre-add, the pitched average pool, the first stem conv (csrc/res2.hip)
RES2_WIDTHS = (32, 64, 128, 224)   # the padded slice widths hvr_res2_conv3x3 has instances for


def res2_pad_width(width):
    """Wp: a Bottle2neck's slice width rounded up to a multiple of 32 (26 / 52 / 104 / 208 -> 32 / 64 / 128 / 224)."""
    return (int(width) + 31) // 32 * 32


def res2_conv3x3_supported(B, H, W, Wp, stride=1, dil=1, dtype=torch.bfloat16, pad=None, ldx=None, x_off=0, ldy=None, y_off=0, add=False, lda=None,
                           add_off=0):
    """True where hvr_res2_conv3x3 has an instance for a slice conv of this shape (res2.hip: bf16 / half, Wp in RES2_WIDTHS, stride 1 / 2,
    pad == dil in {1, 2}, pitches and offsets multiples of 32).  Nothing is launched: placeholder addresses, 1 GiB apart."""
    ldx, ldy, lda = (4 * Wp if v is None else v for v in (ldx, ldy, lda))
    d = Res2ConvDesc(x=_PH, add=(_PH + (2 << 30)) if add else None, y=_PH + (1 << 30), w=_PH, bias=_PH, ldx=ldx, lda=lda, ldy=ldy, x_off=x_off,
                     add_off=add_off, y_off=y_off, B=B, H=H, W=W, Wp=Wp, stride=stride, pad=dil if pad is None else pad, dil=dil, relu=1,
                     dtype=DTYPE_CODES.get(dtype, -1))
    return bool(lib().hvr_res2_conv3x3_supported(ctypes.byref(d)))


class Res2Weight(object):
    """The weight of one branch conv of a Bottle2neck, w [Wp,3,3,Wp] (f32; rows and columns from the real width on are exact zeros), in
    the operand format `dtype`: the form the slice kernel reads, and the form conv2d_nhwc takes on the composite route, whose input
    channels are zero-padded to the Cin multiple of the mode.  Each is built on first use (pack time) and kept."""

    def __init__(self, w, dtype):
        assert w.dim() == 4 and tuple(w.shape[1:3]) == (3, 3) and w.shape[0] == w.shape[3] and w.shape[0] % 32 == 0, tuple(w.shape)
        self.w32, self.dtype, self.Wp = w.detach().float().contiguous(), dtype, int(w.shape[0])
        self.cin = (self.Wp + kstep(dtype) - 1) // kstep(dtype) * kstep(dtype) if dtype != SPLIT else self.Wp
        self._kernel = self._dense = None

    def kernel(self):
        if self._kernel is None:
            if self.dtype not in (torch.bfloat16, torch.float16):
                raise HvrError('hvr_res2_conv3x3 has bf16 and half instances only: the composite route carries %s' % DTYPE_NAMES.get(self.dtype))
            self._kernel = self.w32.to(self.dtype)
        return self._kernel

    def dense(self):
        if self._dense is None:
            self._dense = as_operand(torch.nn.functional.pad(self.w32, (0, self.cin - self.Wp)), self.dtype)
        return self._dense


def _slice_args(t, off, Wp, what):
    assert t.dim() == 4 and t.is_contiguous(), '%s: a contiguous physical NHWC map' % what
    if off < 0 or off + Wp > t.shape[3]:
        raise HvrError('hvr_res2_conv3x3: %s slice [%d, %d) lies outside the map\'s %d channels' % (what, off, off + Wp, t.shape[3]))
    return int(t.shape[3]), int(off)


def res2_conv3x3(x, x_off, w, bias, add=None, add_off=0, out=None, out_off=0, stride=1, dil=1, relu=True, route=None):
    """One branch conv of a Bottle2neck (the rule: include/hvr_hip.h, hvr_res2_conv3x3): the 3x3 conv, pad = dil, of the Wp channels of
    x [B,H,W,Cx] from x_off on -- with `add`, of round(f32(that slice) + f32(add's Wp channels from add_off on)) -- plus bias, ReLU, written
    to the Wp channels of out [B,OH,OW,Cy] from out_off on (out=None: a fresh [B,OH,OW,Wp] map).  w: a Res2Weight, or a [Wp,3,3,Wp]
    tensor (packed on every call: tests and tools).  Returns out.
    route: None = the slice kernel where it has an instance for this shape and format, else 'composite'; 'kernel' / 'composite' force one
    (the forced kernel raises HvrError where it has no instance).  The composite route is made of calls older than the kernel: the
    slice copied out (channels zero-padded to the mode's Cin multiple), the add in f32 and its rounding in torch, conv2d_nhwc, the copy
    into the output slice; it carries f32 and split half.  Neither route touches the host."""
    assert route in (None, 'kernel', 'composite'), route
    _need_cuda(x, bias, add, out)
    rw = w if isinstance(w, Res2Weight) else Res2Weight(w, x.dtype)
    _need_cuda(rw.w32)
    assert rw.dtype == x.dtype, (rw.dtype, x.dtype)
    Wp = rw.Wp
    B, H, W, _ = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out, out_off = torch.empty((B, OH, OW, Wp), dtype=x.dtype, device=x.device), 0
    assert tuple(out.shape[:3]) == (B, OH, OW) and out.dtype == x.dtype, (tuple(out.shape), (B, OH, OW))
    assert add is None or (tuple(add.shape[:3]) == (B, H, W) and add.dtype == x.dtype), 'add has x\'s spatial size and format'
    assert bias.dtype == torch.float32 and bias.numel() == Wp
    ldx, x_off = _slice_args(x, x_off, Wp, 'x')
    ldy, out_off = _slice_args(out, out_off, Wp, 'out')
    lda, add_off = _slice_args(add, add_off, Wp, 'add') if add is not None else (0, 0)
    d = Res2ConvDesc(ldx=ldx, lda=lda, ldy=ldy, x_off=x_off, add_off=add_off, y_off=out_off, B=B, H=H, W=W, Wp=Wp, stride=stride, pad=dil, dil=dil,
                     relu=int(relu), dtype=_dt(x))
    _point(d, x=x, add=add, y=out, bias=bias)
    if route is None:
        d.w = _PH
        route = 'kernel' if Wp in RES2_KERNEL_WIDTHS.get(x.dtype, ()) and lib().hvr_res2_conv3x3_supported(ctypes.byref(d)) else 'composite'
    if route == 'kernel':
        # (the library checks the descriptor before it launches anything: a forced route outside the instance set raises here; f32 and
        # split half have no kernel form of the weight, the library refuses the format before it looks at the address)
        d.w = rw.kernel().data_ptr() if x.dtype in (torch.bfloat16, torch.float16) else _PH
        tag = 'res2conv' if not (_prof and _prof['detail']) else 'res2conv %dx%d %d s%d d%d%s' % (H, W, Wp, stride, dil, '+add' if add is not None else '')
        # bytes it moves: the slice (and the added one) in, the slice out, the weights once
        with _span(tag, float((B * H * W * Wp * (2 if add is not None else 1) + B * OH * OW * Wp + 9 * Wp * Wp) * x.element_size())):
            _check(lib().hvr_res2_conv3x3(ctypes.byref(d), _stream()), 'hvr_res2_conv3x3')
        return out
    xs = x[..., x_off:x_off + Wp]
    if add is not None:
        a = add[..., add_off:add_off + Wp]
        if x.dtype == SPLIT:
            s = cast(cast(xs.contiguous(), torch.float32) + cast(a.contiguous(), torch.float32), SPLIT)
        else:
            s = (xs.float() + a.float()).to(x.dtype)
    else:
        s = xs
    if rw.cin != Wp:
        s = torch.nn.functional.pad(s, (0, rw.cin - Wp))
    y = conv2d_nhwc(s.contiguous(), rw.dense(), bias, relu=relu, stride=stride, pad=dil, dil=dil)
    out[..., out_off:out_off + Wp].copy_(y)
    return out


# The widths at which the automatic route takes the slice kernel, per format (tools/res2_bench.py: the kernel against the composite
# route at the stage shapes of a window).  Every other width, f32 and split half run the composite route.
RES2_KERNEL_WIDTHS = {torch.bfloat16: (32, 64, 128), torch.float16: (32, 64, 128)}


def avgpool_out_hw(H, W, k, stride, pad=0, ceil_mode=False):
    """torch.nn.AvgPool2d's output size."""
    out = []
    for n in (H, W):
        span = n + 2 * pad - k
        o = (-(-span // stride) if ceil_mode else span // stride) + 1
        if ceil_mode and (o - 1) * stride >= n + pad:
            o -= 1
        out.append(o)
    return tuple(out)


def avgpool_nhwc(x, k, stride=1, pad=0, ceil_mode=False, count_include_pad=True, x_off=0, C=None, out=None, out_off=0):
    """k x k average pool (torch.nn.AvgPool2d's sizes and divisors; the rule: include/hvr_hip.h, hvr_avgpool_nhwc) of the C channels of
    x [B,H,W,Cx] from x_off on (C=None: all behind x_off) into the C channels of out [B,OH,OW,Cy] from out_off on (out=None: a fresh
    [B,OH,OW,C] map).  k = 1, stride 1 copies the slice.  Split half is pooled in f32 (cast out and back, as maxpool3x3s2_nhwc)."""
    _need_cuda(x, out)
    assert x.dim() == 4 and x.is_contiguous()
    B, H, W, Cx = x.shape
    C = Cx - x_off if C is None else C
    OH, OW = avgpool_out_hw(H, W, k, stride, pad, ceil_mode)
    if out is None:
        out, out_off = torch.empty((B, OH, OW, C), dtype=x.dtype, device=x.device), 0
    assert out.dim() == 4 and out.is_contiguous() and tuple(out.shape[:3]) == (B, OH, OW) and out.dtype == x.dtype, (tuple(out.shape), (B, OH, OW))
    if x.dtype == SPLIT:
        y = avgpool_nhwc(cast(x[..., x_off:x_off + C].contiguous(), torch.float32), k, stride, pad, ceil_mode, count_include_pad)
        out[..., out_off:out_off + C].copy_(cast(y, SPLIT))
        return out
    d = PoolDesc(x=x.data_ptr(), y=out.data_ptr(), ldx=Cx, ldy=out.shape[3], x_off=x_off, y_off=out_off, B=B, H=H, W=W, C=C, k=k, stride=stride,
                 pad=pad, ceil_mode=int(ceil_mode), count_include_pad=int(count_include_pad), dtype=_dt(x))
    with _span('avgpool', float((B * H * W * C + B * OH * OW * C) * x.element_size())):
        _check(lib().hvr_avgpool_nhwc(ctypes.byref(d), _stream()), 'hvr_avgpool_nhwc')
    return out


def stem3x3s2_first(img, w, bias, dtype, channels=32):
    """The first conv of Res2Net's deep stem (3 -> 32, 3x3 / 2, pad 1, folded BN bias, ReLU) of img [B,3,H,W] f32 NCHW -> physical NHWC
    [B,OH,OW,channels] in the compute format `dtype`; channels 32 onwards are exact zeros (the K padding of the conv that follows).
    w f32 [32,3,3,3] as [n,ky,kx,c], bias f32 [32].  Split half: f32 out, then cast."""
    _need_cuda(img, w, bias)
    assert img.dtype == torch.float32 and img.is_contiguous() and img.shape[1] == 3
    assert w.dtype == torch.float32 and tuple(w.shape) == (32, 3, 3, 3) and w.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == 32
    B, _, H, W = img.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, OH, OW, channels), dtype=torch.float32 if dtype == SPLIT else dtype, device=img.device)
    with _span('stem', 2.0 * B * OH * OW * 32 * 27):
        _check(lib().hvr_stem3x3s2_first(_ptr(img), _ptr(w), _ptr(bias), _ptr(y), B, H, W, channels, _dt(y), _stream()), 'hvr_stem3x3s2_first')
    return cast(y, SPLIT) if dtype == SPLIT else y


def im2col_stem(img, dtype, kp=192):
    """img [B,3,H,W] f32 NCHW -> ([B*OH*OW, kp] patches, OH, OW)."""
    _need_cuda(img)
    assert img.dtype == torch.float32 and img.is_contiguous()
    B, _, H, W = img.shape
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    cols = torch.empty((B * OH * OW, kp), dtype=torch.float32 if dtype == SPLIT else dtype, device=img.device)
    _check(lib().hvr_im2col_stem(_ptr(img), _ptr(cols), B, H, W, kp, _dt(cols), _stream()), 'hvr_im2col_stem')
    return (cast(cols, SPLIT) if dtype == SPLIT else cols), OH, OW   # (split half: through cast(), which applies the activation scale)


def stem_fused(img, wpk, bias):
    """img [B,3,H,W] f32 NCHW -> conv7x7/2 + bias + ReLU + maxpool3x3/2 as physical NHWC bf16 [B,PH,PW,64]."""
    _need_cuda(img, wpk, bias)
    assert img.dtype == torch.float32 and img.is_contiguous() and wpk.dtype in (torch.bfloat16, torch.float16)
    split = wpk.dim() == 4   # [2, 64, 7, 32] half: the hi / lo planes of split-half weights (stem_split_weights)
    assert tuple(wpk.shape) == ((2, 64, 7, 32) if split else (64, 7, 32)) and (not split or wpk.dtype == torch.float16) and wpk.is_contiguous()
    B, _, H, W = img.shape
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (CH + 2 - 3) // 2 + 1, (CW + 2 - 3) // 2 + 1
    out = torch.empty((B, PH, PW, 64), dtype=SPLIT if split else wpk.dtype, device=img.device)
    with _span('stem', 2.0 * B * CH * CW * 64 * 147):
        _check(lib().hvr_stem_fused_dtype(_ptr(img), _ptr(wpk), _ptr(bias), _ptr(out), B, H, W, HVR_F16S if split else _dt(wpk), _stream()),
               'hvr_stem_fused')
    return out


def stem_split_weights(wf):
    """f32 fused-stem weights [64, 7, 32] -> [2, 64, 7, 32] half planes (hi, lo) of the weights x 2^6 x the activation scale: the kernel
    takes 2^6 back, so with the bias x SPLIT_ACT_SCALE (stem_split_bias) its output is a scaled split activation."""
    wf = wf * (SPLIT_WEIGHT_SCALE * SPLIT_ACT_SCALE)
    hi = wf.half()
    lo = (wf - hi.float()).half()
    return torch.stack([hi, lo], 0).contiguous()


def stem_split_bias(b):
    return (b * SPLIT_ACT_SCALE).contiguous()


def maxpool3x3s2_nhwc(x):
    _need_cuda(x)
    if x.dtype == SPLIT:   # pooled in f32 (max does not act per half plane)
        return cast(maxpool3x3s2_nhwc(cast(x, torch.float32)), SPLIT)
    B, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, OH, OW, C), dtype=x.dtype, device=x.device)
    _check(lib().hvr_maxpool3x3s2_nhwc(_ptr(x), _ptr(y), B, H, W, C, _dt(x), _stream()), 'hvr_maxpool3x3s2_nhwc')
    return y


_ws_cache = {}


# Few-row split-K (hvr_gemm_fewrow_workspace_bytes / hvr_conv2d_splitk_workspace_bytes): opt-in, because it changes the f32
# summation order with the batch size -- a frame's rows computed alone would no longer equal the same rows computed in a
# batch bit for bit, a property the cached / look-ahead loops are tested for.  graphs.GraphedStream turns it on for its
# one-frame graphs (the stream loop's latency case); everything else runs the unsplit kernels.
_fewrow = [False]


def fewrow_enabled():
    """True inside `fewrow_split(True)`: convs and products may then run K-sliced, in a summation order that depends on the row count."""
    return _fewrow[0]


@contextlib.contextmanager
def fewrow_split(on=True):
    prev = _fewrow[0]
    _fewrow[0] = bool(on)
    try:
        yield
    finally:
        _fewrow[0] = prev


BIG_TILE_HINT = 16   # gemm_params.h: kBigHint
TWO_LEVEL_HINT = 18  # gemm_params.h: kTwoLevelHint (conv2d_nhwc: two-level accumulation for f32 / split-half operands, else as hint 0)


@contextlib.contextmanager
def throughput_mode(on=True):
    """Launches issued inside prefer CU-time over latency: convs / linear layers whose 288 x 256 tile grid covers only half the
    chip (layer 3: 125 workgroups) still take the big-tile kernel (bigtile.hip) -- for callers that keep several windows in
    flight (bench.py's headline region captures its window graphs inside this).  Same results bit for bit."""
    global TILE_HINT
    prev = TILE_HINT
    if on and TILE_HINT == 0:
        TILE_HINT = BIG_TILE_HINT
    try:
        yield
    finally:
        TILE_HINT = prev


_hip_rt = [None]
_masked_streams = {}   # (device index, first, n) -> (raw handle, ExternalStream): ONE queue per mask, kept for the life of the process


def cu_masked_stream(device, first_cu, n_cus, total_cus=256):
    """A HIP stream whose launches -- direct ones and hipGraph replays issued ON it -- only use `n_cus` of the chip's CUs
    (hipExtStreamCreateWithCUMask, mask bits [first_cu, first_cu + n_cus)).  On MI355X a contiguous range of mask bits is spread
    over all eight XCDs (96 bits = 12 CUs in each: measured in round 3 with a per-CU occupancy probe, profiles/r03_stream_bench.json), and the mask belongs to the stream a graph is replayed on,
    not to the one it was captured on.  Every mask is a hardware queue of its own: a process that creates a dozen of them slows
    every one down (queue oversubscription), so streams are cached per mask.  -> torch.cuda.ExternalStream"""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(first_cu), int(n_cus))
    if key in _masked_streams:
        return _masked_streams[key][1]
    if _hip_rt[0] is None:
        rt = ctypes.CDLL('libamdhip64.so')
        rt.hipExtStreamCreateWithCUMask.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        rt.hipExtStreamCreateWithCUMask.restype = ctypes.c_int
        _hip_rt[0] = rt
    if not (0 <= first_cu and n_cus > 0 and first_cu + n_cus <= total_cus):
        raise HvrError('CU mask [%d, %d) outside [0, %d)' % (first_cu, first_cu + n_cus, total_cus))
    words = (total_cus + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for cu in range(first_cu, first_cu + n_cus):
        mask[cu // 32] |= 1 << (cu % 32)
    handle = ctypes.c_void_p()
    with torch.cuda.device(key[0]):
        rc = _hip_rt[0].hipExtStreamCreateWithCUMask(ctypes.byref(handle), words, mask)
    if rc != 0:
        raise HvrError('hipExtStreamCreateWithCUMask failed (%d)' % rc)
    st = torch.cuda.ExternalStream(handle.value, device=torch.device('cuda', key[0]))
    _masked_streams[key] = (handle, st)
    return st


_ws_captured = set()   # keys whose current buffer was handed out during a stream capture
_ws_retired = []       # replaced buffers a captured graph may still address: never freed


def _workspace(nbytes, device, tag):
    # one buffer per (use, stream): windows enqueued on different HIP streams run concurrently and must not share scratch
    key = (tag, device.index if isinstance(device, torch.device) else str(device), _raw_stream(device if isinstance(device, torch.device) else None))
    ws = _ws_cache.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ws is None or ws.numel() < nbytes:
        if capturing:
            raise HvrError('scratch buffer %r must grow (%d -> %d bytes) inside a stream capture: warm the largest shapes up first'
                           % (tag, 0 if ws is None else ws.numel(), nbytes))
        if ws is not None and key in _ws_captured:
            _ws_retired.append(ws)   # a captured graph holds this address (hvrnet_amd/graphs.py): keep it alive
            _ws_captured.discard(key)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    if capturing:
        _ws_captured.add(key)
    return ws


def relation_fwd(q, k, v, scale, staging=None):
    """softmax(scale * q @ k^T, dim=1) @ v without materialising the f32 logits."""
    _need_cuda(q, k, v)
    Mq, D = q.shape
    Mk = k.shape[0]
    assert k.shape[1] == D and v.shape == (Mk, D) and q.dtype == k.dtype == v.dtype
    o = torch.empty((Mq, D), dtype=q.dtype, device=q.device)
    nbytes = lib().hvr_relation_workspace_bytes(Mq, Mk, D, _dt(q))
    ws = _workspace(nbytes, q.device, 'relation')
    if q.dtype == SPLIT:   # q, k arrive x SPLIT_ACT_SCALE each; v's scale carries over to the output
        scale = float(scale) / (SPLIT_ACT_SCALE * SPLIT_ACT_SCALE)
    with _span('relation_full' if Mq == Mk else 'relation_key', 4.0 * Mq * Mk * D):
        _check(lib().hvr_relation_fwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0),
                                      Mq, Mk, D, float(scale), _dt(q), STAGING if staging is None else staging,
                                      _ptr(ws), ws.numel(), _stream()), 'hvr_relation_fwd')
    return o


def relation_fwd_grouped(q, k, v, scale, groups, staging=None, exact=False):
    """`groups` independent relation problems of one shape in one call (the clips a batched head has in flight): q [G * Mq, D],
    k / v [G * Mk, D] hold the groups' rows back to back (row-strided views are fine: group g starts g * rows * stride(0) elements
    behind group 0) -> o [G * Mq, D], group g's rows = relation_fwd of group g's q / k / v (hvr_relation_fwd_grouped): up to the
    association of the f32 sums by default, bit for bit with exact=True."""
    _need_cuda(q, k, v)
    G = int(groups)
    assert G >= 1 and q.shape[0] % G == 0 and k.shape[0] % G == 0
    Mq, Mk, D = q.shape[0] // G, k.shape[0] // G, q.shape[1]
    assert k.shape[1] == D and v.shape == k.shape and q.dtype == k.dtype == v.dtype
    if G == 1:
        return relation_fwd(q, k, v, scale, staging)
    o = torch.empty((G * Mq, D), dtype=q.dtype, device=q.device)
    nbytes = lib().hvr_relation_grouped_workspace_bytes(G, Mq, Mk, D, _dt(q))
    ws = _workspace(nbytes, q.device, 'relation_grouped')
    if q.dtype == SPLIT:
        scale = float(scale) / (SPLIT_ACT_SCALE * SPLIT_ACT_SCALE)
    with _span('relation_full' if Mq == Mk else 'relation_key', 4.0 * G * Mq * Mk * D):
        _check(lib().hvr_relation_fwd_grouped(_ptr(q), q.stride(0), Mq * q.stride(0), _ptr(k), k.stride(0), Mk * k.stride(0),
                                              _ptr(v), v.stride(0), Mk * v.stride(0), _ptr(o), o.stride(0), Mq * o.stride(0), G,
                                              Mq, Mk, D, float(scale), _dt(q), STAGING if staging is None else staging, int(bool(exact)),
                                              _ptr(ws), ws.numel(), _stream()), 'hvr_relation_fwd_grouped')
    return o


def relation_ldp(Mk):
    """Row length of the relation's probability matrix: keys padded to a multiple of 128."""
    return (Mk + 127) // 128 * 128


def relation_probs(q, k, scale, staging=None, out=None):
    """softmax(scale * q @ k^T, dim=1) as a [Mq, ldp] matrix of q's dtype (padding columns zero); `out`: a contiguous [Mq, ldp]
    tensor to write into (every element is overwritten)."""
    _need_cuda(q, k)
    Mq, D = q.shape
    Mk = k.shape[0]
    ldp = relation_ldp(Mk)
    P = _out(out, (Mq, ldp), q.dtype, q.device)
    ws = _workspace(lib().hvr_relation_probs_workspace_bytes(Mq, Mk), q.device, 'relation_probs')
    _check(lib().hvr_relation_probs(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(P), ldp, Mq, Mk, D, float(scale), _dt(q),
                                    STAGING if staging is None else staging, _ptr(ws), ws.numel(), _stream()), 'hvr_relation_probs')
    return P


def relation_dscore(P, dP, dO, O, scale):
    """scale * P * (dP - rowsum(dO * O)): gradient w.r.t. the un-scaled logits q @ k^T, same shape / dtype as P."""
    _need_cuda(P, dP, dO, O)
    assert P.shape == dP.shape and P.is_contiguous() and dP.is_contiguous() and dO.stride(1) == 1 and O.stride(1) == 1
    dS = torch.empty_like(P)
    _check(lib().hvr_relation_dscore(_ptr(P), _ptr(dP), _ptr(dO), dO.stride(0), _ptr(O), O.stride(0), _ptr(dS), P.shape[0],
                                     P.shape[1], dO.shape[1], float(scale), _dt(P), _stream()), 'hvr_relation_dscore')
    return dS


def im2col_nhwc(x, KH, KW, pad, dil):
    """x [B,H,W,Cin] -> patch matrix [B*OH*OW, KH*KW*Cin] (stride 1, zero padding)."""
    _need_cuda(x)
    x = x.contiguous()
    B, H, W, Cin = x.shape
    OH, OW = H + 2 * pad - dil * (KH - 1), W + 2 * pad - dil * (KW - 1)
    cols = torch.empty((B * OH * OW, KH * KW * Cin), dtype=x.dtype, device=x.device)
    _check(lib().hvr_im2col_nhwc(_ptr(x), _ptr(cols), B, H, W, Cin, KH, KW, pad, dil, _dt(x), _stream()), 'hvr_im2col_nhwc')
    return cols


def scale_rows(w, scale):
    """[R, ...] * scale[R] per leading row (f32 scale)."""
    _need_cuda(w, scale)
    w = w.contiguous()
    out = torch.empty_like(w)
    R = w.shape[0]
    _check(lib().hvr_scale_rows(_ptr(w), _ptr(scale.float().contiguous()), _ptr(out), R, w.numel() // R, _dt(w), _stream()), 'hvr_scale_rows')
    return out


def sgd_step(param_flat, grad_flat, momentum_buf, lr, momentum, weight_decay, grad_scale=1.0, max_norm=0.0, first_step=False):
    """In-place SGD-with-momentum update of a flat f32 parameter buffer (see hvr_sgd_step in include/hvr_hip.h)."""
    _need_cuda(param_flat, grad_flat, momentum_buf)
    assert param_flat.dtype == grad_flat.dtype == momentum_buf.dtype == torch.float32
    assert param_flat.is_contiguous() and grad_flat.is_contiguous() and momentum_buf.is_contiguous()
    assert param_flat.numel() == grad_flat.numel() == momentum_buf.numel()
    ws = _workspace(lib().hvr_sgd_workspace_bytes(), param_flat.device, 'sgd')
    _check(lib().hvr_sgd_step(_ptr(param_flat), _ptr(grad_flat), _ptr(momentum_buf), param_flat.numel(), float(lr), float(momentum),
                              float(weight_decay), float(grad_scale), float(max_norm), _ptr(ws), ws.numel(), int(first_step),
                              _stream()), 'hvr_sgd_step')


def relu_bwd(dy, y):
    """dy where y > 0 else 0 (y: the output of a GEMM epilogue with relu=True)."""
    _need_cuda(dy, y)
    dy, y = dy.contiguous(), y.contiguous()
    assert dy.shape == y.shape and dy.dtype == y.dtype and dy.numel() % 4 == 0
    dz = torch.empty_like(dy)
    _check(lib().hvr_relu_bwd(_ptr(dy), _ptr(y), _ptr(dz), dy.numel(), _dt(dy), _stream()), 'hvr_relu_bwd')
    return dz


def relu_bwd_t(dy, y, ldt, dzt_out=None):
    """(dz, dzt): dz = dy where y > 0 ([R, C]) and its transpose [C, ldt] (columns R.. zero) from one pass (bf16 / half).
    dzt_out: a contiguous [C, ldt] tensor to write the transpose into (a slot of a stage's weight-gradient slab)."""
    _need_cuda(dy, y)
    dy, y = dy.contiguous(), y.contiguous()
    assert dy.dim() == 2 and dy.shape == y.shape and dy.dtype == y.dtype
    R, C = dy.shape
    dz = torch.empty_like(dy)
    dzt = _out(dzt_out, (C, ldt), dy.dtype, dy.device)
    _check(lib().hvr_relu_bwd_t(_ptr(dy), _ptr(y), _ptr(dz), _ptr(dzt), ldt, R, C, _dt(dy), _stream()), 'hvr_relu_bwd_t')
    return dz, dzt


def im2col_t(x, KH, KW, pad, dil, ldt, out=None):
    """x [B,H,W,Cin] (NHWC, bf16 / half) -> the TRANSPOSED patch matrix [KH*KW*Cin, ldt] of a stride-1 conv (columns B*OH*OW.. zero)."""
    _need_cuda(x)
    x = x.contiguous()
    B, H, W, Cin = x.shape
    out = _out(out, (KH * KW * Cin, ldt), x.dtype, x.device)
    _check(lib().hvr_im2col_t(_ptr(x), _ptr(out), ldt, B, H, W, Cin, KH, KW, pad, dil, _dt(x), _stream()), 'hvr_im2col_t')
    return out


def colsum(dy, out=None):
    """[M, N] -> f32 [N] column sums (bias gradient); out: a contiguous f32 [N] tensor to write into."""
    _need_cuda(dy)
    assert dy.dim() == 2 and dy.stride(1) == 1
    db = _out(out, (dy.shape[1],), torch.float32, dy.device)
    nbytes = lib().hvr_colsum_workspace_bytes(dy.shape[0], dy.shape[1])
    ws = _workspace(nbytes, dy.device, 'colsum') if nbytes else None
    _check(lib().hvr_colsum(_ptr(dy), _ptr(db), dy.shape[0], dy.shape[1], dy.stride(0), _dt(dy), _ptr(ws), nbytes, _stream()), 'hvr_colsum')
    return db


def pack_conv_weight(w, scale, dtype):
    """nn.Conv2d weight [Cout,Cin,KH,KW] f32 * scale[Cout] -> [Cout,KH,KW,Cin] in `dtype` (the conv kernel's operand)."""
    _need_cuda(w, scale)
    assert w.dtype == torch.float32 and w.is_contiguous() and scale.dtype == torch.float32 and scale.is_contiguous()
    Cout, Cin, KH, KW = w.shape
    out = torch.empty((Cout, KH, KW, Cin), dtype=dtype, device=w.device)
    _check(lib().hvr_pack_conv_weight(_ptr(w), _ptr(scale), _ptr(out), Cout, Cin, KH, KW, _dt(out), _stream()), 'hvr_pack_conv_weight')
    return out


class PackItem(ctypes.Structure):          # hvr_pack_item
    _fields_ = [('w', ctypes.c_void_p), ('scale', ctypes.c_void_p), ('out', ctypes.c_void_p), ('first', ctypes.c_int64),
                ('Cout', ctypes.c_int32), ('Cin', ctypes.c_int32), ('KK', ctypes.c_int32), ('pad_', ctypes.c_int32)]


class TransposeItem(ctypes.Structure):     # hvr_transpose_item
    _fields_ = [('src', ctypes.c_void_p), ('dst', ctypes.c_void_p), ('lds', ctypes.c_int64), ('ldd', ctypes.c_int64),
                ('R', ctypes.c_int32), ('C', ctypes.c_int32), ('first_tile', ctypes.c_int32), ('tiles_c', ctypes.c_int32),
                ('dcols', ctypes.c_int32), ('pad_', ctypes.c_int32)]


def items_to_device(items, device):
    """A list of ctypes structures -> a uint8 device tensor holding the array (the descriptor tables of the *_multi entry points)."""
    arr = (type(items[0]) * len(items))(*items)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def pack_conv_weights_multi(items_dev, n, total, dtype):
    code = {torch.bfloat16: HVR_BF16, torch.float16: HVR_F16}[dtype]
    _check(lib().hvr_pack_conv_weights_multi(_ptr(items_dev), n, total, code, _stream()), 'hvr_pack_conv_weights_multi')


def transpose_multi(items_dev, n, tiles):
    _check(lib().hvr_transpose_multi(_ptr(items_dev), n, tiles, _stream()), 'hvr_transpose_multi')


def unpack_conv_wgrads_multi(items_dev, n, total, accumulate=True):
    """hvr_unpack_conv_wgrad for a device table of layers (PackItem: w = the parameter-layout gradient to add to, scale, out = the f32
    product) in one launch."""
    _check(lib().hvr_unpack_conv_wgrads_multi(_ptr(items_dev), n, total, int(accumulate), _stream()), 'hvr_unpack_conv_wgrads_multi')


def unpack_conv_wgrad(dw, scale, shape, accumulate_into=None):
    """dW_eff [Cout, KH*KW*Cin] f32 * scale[Cout] -> [Cout,Cin,KH,KW] f32 (the nn.Conv2d parameter's layout); with
    `accumulate_into` (a contiguous f32 tensor of that shape, e.g. the parameter's .grad) the result is added to it in place."""
    _need_cuda(dw, scale)
    Cout, Cin, KH, KW = shape
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == Cout * Cin * KH * KW
    if accumulate_into is not None:
        out = accumulate_into
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(shape)
    else:
        out = torch.empty(shape, dtype=torch.float32, device=dw.device)
    _check(lib().hvr_unpack_conv_wgrad(_ptr(dw), _ptr(scale), _ptr(out), Cout, Cin, KH, KW, int(accumulate_into is not None), _stream()),
           'hvr_unpack_conv_wgrad')
    return out


def _loss_operands(labels, label_weights, bbox_targets, bbox_weights, n):
    """The per-row (per-anchor) operands of the loss kernels as contiguous int64 / f32 tensors of the right length.  The results are
    NAMED by the caller until after the launch: a converted copy passed as `_ptr(t.float())` dies with the expression, and the
    caching allocator hands its block to the next temporary before the kernel has read it."""
    assert labels.numel() == label_weights.numel() == n, 'labels / label_weights: one value per anchor (rows * A) or row'
    assert bbox_targets.numel() == bbox_weights.numel() == 4 * n, 'bbox_targets / bbox_weights: four values per anchor or row'
    return labels.contiguous(), label_weights.float().contiguous(), bbox_targets.float().contiguous(), bbox_weights.float().contiguous()


def det_loss(logits, cls_off, reg_off, ncls, labels, label_weights, bbox_targets, bbox_weights, beta=1.0, w_cls=1.0, w_bbox=1.0):
    """BBoxHead.loss on a fused [R, ld] f32 logit matrix -> (out3 = [loss_cls, loss_bbox, acc] f32, dlogits [R, ld] f32)."""
    _need_cuda(logits, labels, label_weights, bbox_targets, bbox_weights)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.long
    labels, lw, bt, bw = _loss_operands(labels, label_weights, bbox_targets, bbox_weights, logits.shape[0])
    out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    _check(lib().hvr_det_loss(_ptr(logits), logits.shape[1], cls_off, reg_off, ncls, _ptr(labels), _ptr(lw), _ptr(bt), _ptr(bw),
                              logits.shape[0], float(beta), float(w_cls), float(w_bbox), _ptr(out3), _ptr(dlogits), _stream()),
           'hvr_det_loss')
    return out3, dlogits



# ---- training targets (include/hvr_hip.h "Training targets") ----
def max_iou_assign(boxes, gts, pos_iou_thr, neg_iou_thr, min_pos_iou, valid=None):
    """boxes [n, >=4] f32, gts [k,4] f32, valid [n] uint8/bool or None -> (gt_inds int64 [n], max_overlaps f32 [n]).
    neg_iou_thr: float (background = [0, thr)) or a (lo, hi) pair."""
    _need_cuda(boxes, gts, valid)
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.stride(1) == 1 and boxes.shape[1] >= 4
    gts = gts.contiguous().float()
    n, k = boxes.shape[0], gts.shape[0]
    if n == 0 or k == 0:
        raise ValueError('No gt or bboxes')  # max_iou_assigner.py:77-78
    lo, hi = (0.0, float(neg_iou_thr)) if isinstance(neg_iou_thr, (int, float)) else (float(neg_iou_thr[0]), float(neg_iou_thr[1]))
    if valid is not None:
        valid = valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else valid.contiguous()
        assert valid.dtype == torch.uint8 and valid.numel() == n
    gt_inds = torch.empty(n, dtype=torch.long, device=boxes.device)
    max_ov = torch.empty(n, dtype=torch.float32, device=boxes.device)
    nbytes = lib().hvr_max_iou_assign_workspace_bytes(n, k)
    ws = _workspace(nbytes, boxes.device, 'assign')
    _check(lib().hvr_max_iou_assign(_ptr(boxes), boxes.stride(0), n, _ptr(gts), k, _ptr(valid), float(pos_iou_thr), lo, hi,
                                    float(min_pos_iou), _ptr(gt_inds), _ptr(max_ov), _ptr(ws), nbytes, _stream()), 'hvr_max_iou_assign')
    return gt_inds, max_ov


def sample_pos_neg(cls, keys, num, num_expected_pos, neg_pos_ub=-1.0):
    """cls int64 [n] (>0 positive, ==0 negative), keys f32 [n] -> (inds int64 [num]: positives then negatives, counts int32 [2]).
    The smallest keys win, compared numerically (-0.0 ties with +0.0; ties go to the lower index; +-inf are ordinary values);
    NaN keys are unspecified.  Rows of inds behind counts[0] + counts[1] are left unwritten.  neg_pos_ub >= 0 caps the negatives
    at int(neg_pos_ub * max(1, counts[0])), evaluated in double on this Python float (base_sampler.py:70)."""
    _need_cuda(cls, keys)
    assert cls.dtype == torch.long and cls.is_contiguous() and keys.dtype == torch.float32 and keys.is_contiguous()
    assert cls.numel() == keys.numel()
    inds = torch.empty(int(num), dtype=torch.long, device=cls.device)
    counts = torch.empty(2, dtype=torch.int32, device=cls.device)
    _check(lib().hvr_sample_pos_neg(_ptr(cls), _ptr(keys), cls.numel(), int(num), int(num_expected_pos), float(neg_pos_ub), _ptr(inds),
                                    _ptr(counts), _stream()), 'hvr_sample_pos_neg')
    return inds, counts


def box_targets(boxes, gts, gt_labels, gt_inds, inds, counts, means, stds, pos_weight=-1.0, scatter=False):
    """-> (labels int64, label_weights, bbox_targets [.,4], bbox_weights [.,4]) with n rows (scatter) or num rows."""
    _need_cuda(boxes, gts, gt_labels, gt_inds, inds, counts)
    assert boxes.dtype == torch.float32 and boxes.stride(1) == 1 and gt_inds.dtype == torch.long and inds.dtype == torch.long
    gts = gts.contiguous().float()
    n, num = boxes.shape[0], inds.numel()
    rows = n if scatter else num
    dev = boxes.device
    labels = torch.empty(rows, dtype=torch.long, device=dev)
    label_w = torch.empty(rows, dtype=torch.float32, device=dev)
    bbox_t = torch.empty((rows, 4), dtype=torch.float32, device=dev)
    bbox_w = torch.empty((rows, 4), dtype=torch.float32, device=dev)
    m4, s4 = (ctypes.c_float * 4)(*[float(v) for v in means]), (ctypes.c_float * 4)(*[float(v) for v in stds])
    gl = gt_labels.contiguous() if gt_labels is not None else None
    _check(lib().hvr_box_targets(_ptr(boxes), boxes.stride(0), n, _ptr(gts), _ptr(gl), _ptr(gt_inds.contiguous()), _ptr(inds),
                                 _ptr(counts), num, ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(s4, ctypes.c_void_p),
                                 float(pos_weight), int(bool(scatter)), _ptr(labels), _ptr(label_w), _ptr(bbox_t), _ptr(bbox_w),
                                 _stream()), 'hvr_box_targets')
    return labels, label_w, bbox_t, bbox_w


def rpn_loss(o, A, labels, label_weights, bbox_targets, bbox_weights, counts, beta):
    """o [rows, ldo] f32 (A objectness logits then 4A deltas per row) -> (out2 = [loss_rpn_cls, loss_rpn_bbox], d_o like o)."""
    _need_cuda(o, labels, label_weights, bbox_targets, bbox_weights, counts)
    assert o.dtype == torch.float32 and o.dim() == 2 and o.is_contiguous() and labels.dtype == torch.long
    rows = o.shape[0]
    assert A >= 1 and o.shape[1] >= 5 * A and counts.dtype == torch.int32 and counts.numel() == 2
    labels, lw, bt, bw = _loss_operands(labels, label_weights, bbox_targets, bbox_weights, rows * A)
    counts = counts.contiguous()
    out2 = torch.empty(2, dtype=torch.float32, device=o.device)
    d_o = torch.empty_like(o)
    _check(lib().hvr_rpn_loss(_ptr(o), o.shape[1], int(A), rows, _ptr(labels), _ptr(lw), _ptr(bt), _ptr(bw), _ptr(counts),
                              float(beta), _ptr(out2), _ptr(d_o), _stream()), 'hvr_rpn_loss')
    return out2, d_o


# ---- sigmoid focal loss (csrc/focal.hip; the rule: include/hvr_hip.h "Sigmoid focal loss")
def _focal_logits(logits, targets, what, dtypes):
    """(N, C, ldl) of a logit matrix [N, C] whose rows are contiguous (any row pitch >= C) with its int64 targets [N]."""
    assert logits.dim() == 2 and logits.dtype in dtypes, '%s: logits [N, C] in %s, got %s %s' % (what, dtypes, logits.dtype, tuple(logits.shape))
    N, C = logits.shape
    assert N >= 1 and C >= 1, '%s: empty logits %s' % (what, tuple(logits.shape))
    assert logits.stride(1) == 1 or C == 1, '%s: the columns of a row must be contiguous' % what
    assert targets.dtype == torch.long and targets.is_contiguous() and targets.numel() == N, '%s: one contiguous int64 target per row' % what
    return N, C, (logits.stride(0) if N > 1 else max(logits.stride(0), C))


_FOCAL_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def sigmoid_focal_loss_fwd(logits, targets, gamma, alpha):
    """logits [N, C] f32 / bf16 / half (rows contiguous, any pitch), targets int64 [N] -> loss f32 [N, C]."""
    _need_cuda(logits, targets)
    N, C, ldl = _focal_logits(logits, targets, 'sigmoid_focal_loss_fwd', _FOCAL_DTYPES)
    loss = torch.empty((N, C), dtype=torch.float32, device=logits.device)
    _check(lib().hvr_sigmoid_focal_loss_fwd(_ptr(logits), ldl, _ptr(targets), N, C, float(gamma), float(alpha), _dt(logits), _ptr(loss), _stream()),
           'hvr_sigmoid_focal_loss_fwd')
    return loss


def sigmoid_focal_loss_bwd(logits, targets, d_loss, gamma, alpha):
    """-> d_logits f32 [N, C] = dl/dx * d_loss (d_loss f32 [N, C] contiguous)."""
    _need_cuda(logits, targets, d_loss)
    N, C, ldl = _focal_logits(logits, targets, 'sigmoid_focal_loss_bwd', _FOCAL_DTYPES)
    assert d_loss.dtype == torch.float32 and d_loss.is_contiguous() and tuple(d_loss.shape) == (N, C)
    d_logits = torch.empty((N, C), dtype=torch.float32, device=logits.device)
    _check(lib().hvr_sigmoid_focal_loss_bwd(_ptr(logits), ldl, _ptr(targets), _ptr(d_loss), N, C, float(gamma), float(alpha), _dt(logits),
                                            _ptr(d_logits), _stream()), 'hvr_sigmoid_focal_loss_bwd')
    return d_logits


def focal_loss_splits(N, C):
    """The workgroups (one f32 partial each) the reduced form cuts N rows of C columns into: a function of the shape only."""
    return int(lib().hvr_focal_loss_splits(int(N), int(C)))


def focal_loss(logits, targets, weight=None, gamma=2.0, alpha=0.25, loss_weight=1.0, avg=1.0, counts=None, ws=None):
    """The reduced form in one launch pair: logits f32 [N, C] (rows contiguous, pitch ldl), targets int64 [N], weight f32 [N] or None
    -> (out1 f32 [1] = loss_weight / avg * sum_n w[n] sum_c l[n][c], d_logits f32 [N, ldl] = loss_weight / avg * w[n] * dl/dx, pitch
    columns zero).  avg: a float, or with counts (int32 on the device) max(counts[0], 1) read there.  ws: a uint8 workspace to use in
    place of a fresh one (a test hands a short one in)."""
    _need_cuda(logits, targets, weight, counts, ws)
    N, C, ldl = _focal_logits(logits, targets, 'focal_loss', (torch.float32,))
    if weight is not None:
        assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == N, 'focal_loss: one contiguous f32 weight per row'
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 1
    nbytes = lib().hvr_focal_loss_workspace_bytes(N, C)
    if ws is None:   # a fresh tensor of torch's allocator (a few KB, stream-ordered), so the call can be captured in a graph on any stream
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=logits.device)
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    given = ws.numel()
    out1 = torch.empty(1, dtype=torch.float32, device=logits.device)
    d_logits = torch.empty((N, ldl), dtype=torch.float32, device=logits.device)
    _check(lib().hvr_focal_loss(_ptr(logits), ldl, _ptr(targets), _ptr(weight), N, C, float(gamma), float(alpha), float(loss_weight), float(avg),
                                _ptr(counts), _ptr(ws), given, _ptr(out1), _ptr(d_logits), _stream()), 'hvr_focal_loss')
    return out1, d_logits


def rpn_focal_loss(o, A, labels, label_weights, bbox_targets, bbox_weights, counts, beta, gamma, alpha, w_cls=1.0, w_bbox=1.0):
    """rpn_loss for a sampling-free head: o [rows, ldo] f32 -> (out2 = [loss_rpn_cls, loss_rpn_bbox], d_o like o); focal rule on the
    objectness logits, both terms over max(counts[0], 1)."""
    _need_cuda(o, labels, label_weights, bbox_targets, bbox_weights, counts)
    assert o.dtype == torch.float32 and o.dim() == 2 and o.is_contiguous() and labels.dtype == torch.long
    rows = o.shape[0]
    assert A >= 1 and o.shape[1] >= 5 * A and counts.dtype == torch.int32 and counts.numel() == 2
    labels, lw, bt, bw = _loss_operands(labels, label_weights, bbox_targets, bbox_weights, rows * A)
    counts = counts.contiguous()
    out2 = torch.empty(2, dtype=torch.float32, device=o.device)
    d_o = torch.empty_like(o)
    _check(lib().hvr_rpn_focal_loss(_ptr(o), o.shape[1], int(A), rows, _ptr(labels), _ptr(lw), _ptr(bt), _ptr(bw), _ptr(counts), float(beta),
                                    float(gamma), float(alpha), float(w_cls), float(w_bbox), _ptr(out2), _ptr(d_o), _stream()), 'hvr_rpn_focal_loss')
    return out2, d_o


# ---- regression, IoU and GHM losses (csrc/reg_loss.hip, csrc/ghm.hip; the rules: include/hvr_hip.h)
REG_RULES = dict(smooth_l1=0, balanced_l1=1, mse=2)
BOX_RULES = dict(iou=0, bounded_iou=1)


def _reg_pair(pred, target, what):
    """(N, D, ldp) of pred f32 [N, D] (rows contiguous, any row pitch >= D) and a dense f32 target of the same shape."""
    assert pred.dim() == 2 and pred.dtype == torch.float32 and pred.numel() > 0, '%s: pred f32 [N, D], got %s %s' % (what, pred.dtype, tuple(pred.shape))
    N, D = pred.shape
    assert pred.stride(1) == 1 or D == 1, '%s: pred rows must be contiguous' % what
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (N, D), '%s: target f32 [N, D] contiguous' % what
    return N, D, (pred.stride(0) if N > 1 else max(pred.stride(0), D))


def _dense(t, shape, what):
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), '%s: f32 %s contiguous, got %s %s' % (
        what, tuple(shape), t.dtype, tuple(t.shape))


def _loss_ws(nbytes, ws, device):
    if ws is None:   # a fresh tensor of torch's allocator (stream-ordered), so the call can be captured in a graph on any stream
        ws = torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    return ws


def _avg_counts(counts):
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 1
    return counts


def reg_loss_fwd(rule, pred, target, beta=1.0, alpha=0.5, gamma=1.5):
    """rule 'smooth_l1' / 'balanced_l1' / 'mse': pred f32 [N, D] (any row pitch), target f32 [N, D] -> loss f32 [N, D]."""
    _need_cuda(pred, target)
    N, D, ldp = _reg_pair(pred, target, 'reg_loss_fwd')
    loss = torch.empty((N, D), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_reg_loss_fwd(REG_RULES[rule], _ptr(pred), ldp, _ptr(target), N, D, float(beta), float(alpha), float(gamma), _ptr(loss),
                                  _stream()), 'hvr_reg_loss_fwd')
    return loss


def reg_loss_bwd(rule, pred, target, d_loss, beta=1.0, alpha=0.5, gamma=1.5):
    """-> d_pred f32 [N, D] = dl/dpred * d_loss (d_loss f32 [N, D] contiguous)."""
    _need_cuda(pred, target, d_loss)
    N, D, ldp = _reg_pair(pred, target, 'reg_loss_bwd')
    _dense(d_loss, (N, D), 'reg_loss_bwd: d_loss')
    d_pred = torch.empty((N, D), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_reg_loss_bwd(REG_RULES[rule], _ptr(pred), ldp, _ptr(target), _ptr(d_loss), N, D, float(beta), float(alpha), float(gamma),
                                  _ptr(d_pred), _stream()), 'hvr_reg_loss_bwd')
    return d_pred


def reg_loss_splits(N, D):
    return int(lib().hvr_reg_loss_splits(int(N), int(D)))


def reg_loss(rule, pred, target, weight=None, beta=1.0, alpha=0.5, gamma=1.5, loss_weight=1.0, avg=1.0, counts=None, ws=None):
    """The reduced form in one pass: -> (out1 f32 [1] = loss_weight / avg * sum w l, d_pred f32 [N, D] = loss_weight / avg * w * dl/dpred).
    weight f32 [N, D] or None.  avg: a float, or with counts (int32 on the device) max(counts[0], 1) read there."""
    _need_cuda(pred, target, weight, counts, ws)
    N, D, ldp = _reg_pair(pred, target, 'reg_loss')
    if weight is not None:
        _dense(weight, (N, D), 'reg_loss: weight')
    counts = _avg_counts(counts)
    ws = _loss_ws(lib().hvr_reg_loss_workspace_bytes(N, D), ws, pred.device)
    out1 = torch.empty(1, dtype=torch.float32, device=pred.device)
    d_pred = torch.empty((N, D), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_reg_loss(REG_RULES[rule], _ptr(pred), ldp, _ptr(target), _ptr(weight), N, D, float(beta), float(alpha), float(gamma),
                              float(loss_weight), float(avg), _ptr(counts), _ptr(ws), ws.numel(), _ptr(out1), _ptr(d_pred), _stream()), 'hvr_reg_loss')
    return out1, d_pred


def _box_pair(pred, target, what):
    assert pred.dim() == 2 and pred.shape[1] == 4 and pred.shape[0] > 0 and pred.dtype == torch.float32 and pred.is_contiguous(), \
        '%s: pred f32 [n, 4] contiguous, got %s %s' % (what, pred.dtype, tuple(pred.shape))
    _dense(target, pred.shape, what + ': target')
    return pred.shape[0]


def _box_loss_shape(rule, n):
    return (n,) if rule == 'iou' else (n, 4)


def box_loss_fwd(rule, pred, target, beta=0.2, eps=1e-3):
    """rule 'iou' / 'bounded_iou': pred, target f32 [n, 4] -> loss f32 [n] / [n, 4]."""
    _need_cuda(pred, target)
    n = _box_pair(pred, target, 'box_loss_fwd')
    loss = torch.empty(_box_loss_shape(rule, n), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_box_loss_fwd(BOX_RULES[rule], _ptr(pred), _ptr(target), n, float(beta), float(eps), _ptr(loss), _stream()), 'hvr_box_loss_fwd')
    return loss


def box_loss_bwd(rule, pred, target, d_loss, beta=0.2, eps=1e-3):
    """-> d_pred f32 [n, 4] (d_loss in the loss's shape)."""
    _need_cuda(pred, target, d_loss)
    n = _box_pair(pred, target, 'box_loss_bwd')
    _dense(d_loss, _box_loss_shape(rule, n), 'box_loss_bwd: d_loss')
    d_pred = torch.empty((n, 4), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_box_loss_bwd(BOX_RULES[rule], _ptr(pred), _ptr(target), _ptr(d_loss), n, float(beta), float(eps), _ptr(d_pred), _stream()),
           'hvr_box_loss_bwd')
    return d_pred


def box_loss_splits(n):
    return int(lib().hvr_box_loss_splits(int(n)))


def box_loss(rule, pred, target, weight=None, beta=0.2, eps=1e-3, loss_weight=1.0, avg=1.0, counts=None, ws=None):
    """The reduced form: -> (out1 f32 [1], d_pred f32 [n, 4]).  weight f32 in the loss's shape ([n] for 'iou', [n, 4] for 'bounded_iou') or None."""
    _need_cuda(pred, target, weight, counts, ws)
    n = _box_pair(pred, target, 'box_loss')
    if weight is not None:
        _dense(weight, _box_loss_shape(rule, n), 'box_loss: weight')
    counts = _avg_counts(counts)
    ws = _loss_ws(lib().hvr_box_loss_workspace_bytes(n), ws, pred.device)
    out1 = torch.empty(1, dtype=torch.float32, device=pred.device)
    d_pred = torch.empty((n, 4), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_box_loss(BOX_RULES[rule], _ptr(pred), _ptr(target), _ptr(weight), n, float(beta), float(eps), float(loss_weight), float(avg),
                              _ptr(counts), _ptr(ws), ws.numel(), _ptr(out1), _ptr(d_pred), _stream()), 'hvr_box_loss')
    return out1, d_pred


def ghm_splits(N, C):
    return int(lib().hvr_ghm_splits(int(N), int(C)))


def ghm_workspace_views(ws, bins):
    """(counts int32 [bins], w f32 [bins], tot f32 [1], n int32 [1]) views of a GHM workspace (the layout: include/hvr_hip.h)."""
    wi, wf = ws[:768].view(torch.int32), ws[:768].view(torch.float32)
    return wi[:bins], wf[64:64 + bins], wf[128:129], wi[129:130]


def _ghm_common(pred, edges, bins, momentum, acc_sum, what):
    assert pred.dim() == 2 and pred.dtype == torch.float32 and pred.is_contiguous() and pred.numel() > 0, '%s: pred f32 [N, C] contiguous' % what
    _dense(edges, (bins + 1,), what + ': edges')
    if momentum > 0:
        _dense(acc_sum, (bins,), what + ': acc_sum')
    return pred.shape


def ghmc_loss(logits, target, weight, edges, momentum=0.0, acc_sum=None, loss_weight=1.0, ws=None):
    """logits f32 [N, C]; target f32 [N, C] with weight f32 [N, C], or int64 labels [N] (label k >= 1 marks column k - 1) with weight
    f32 [N] per row -> (out1 f32 [1], d_logits f32 [N, C], ws); acc_sum f32 [bins] is updated in place when momentum > 0."""
    _need_cuda(logits, target, weight, edges, acc_sum, ws)
    bins = edges.numel() - 1
    N, C = _ghm_common(logits, edges, bins, momentum, acc_sum, 'ghmc_loss')
    by_label = target.dtype == torch.long
    if by_label:
        assert target.is_contiguous() and tuple(target.shape) == (N,), 'ghmc_loss: int64 labels [N]'
        _dense(weight, (N,), 'ghmc_loss: label weights')
    else:
        _dense(target, (N, C), 'ghmc_loss: target')
        _dense(weight, (N, C), 'ghmc_loss: weight')
    ws = _loss_ws(lib().hvr_ghm_workspace_bytes(N, C), ws, logits.device)
    out1 = torch.empty(1, dtype=torch.float32, device=logits.device)
    d = torch.empty((N, C), dtype=torch.float32, device=logits.device)
    _check(lib().hvr_ghmc_loss(_ptr(logits), None if by_label else _ptr(target), _ptr(target) if by_label else None, _ptr(weight), int(by_label),
                               N, C, _ptr(edges), bins, float(momentum), _ptr(acc_sum) if momentum > 0 else None, float(loss_weight), _ptr(ws),
                               ws.numel(), _ptr(out1), _ptr(d), _stream()), 'hvr_ghmc_loss')
    return out1, d, ws


def ghmr_loss(pred, target, weight, edges, mu=0.02, momentum=0.0, acc_sum=None, loss_weight=1.0, ws=None):
    """pred, target, weight f32 [N, C] -> (out1 f32 [1], d_pred f32 [N, C], ws); acc_sum as in ghmc_loss."""
    _need_cuda(pred, target, weight, edges, acc_sum, ws)
    bins = edges.numel() - 1
    N, C = _ghm_common(pred, edges, bins, momentum, acc_sum, 'ghmr_loss')
    _dense(target, (N, C), 'ghmr_loss: target')
    _dense(weight, (N, C), 'ghmr_loss: weight')
    ws = _loss_ws(lib().hvr_ghm_workspace_bytes(N, C), ws, pred.device)
    out1 = torch.empty(1, dtype=torch.float32, device=pred.device)
    d = torch.empty((N, C), dtype=torch.float32, device=pred.device)
    _check(lib().hvr_ghmr_loss(_ptr(pred), _ptr(target), _ptr(weight), N, C, float(mu), _ptr(edges), bins, float(momentum),
                               _ptr(acc_sum) if momentum > 0 else None, float(loss_weight), _ptr(ws), ws.numel(), _ptr(out1), _ptr(d), _stream()),
           'hvr_ghmr_loss')
    return out1, d, ws


def ce_rows(logits, cls_off, ncls, labels):
    """per-row softmax cross entropy of logits[:, cls_off:cls_off+ncls] -> f32 [R]."""
    _need_cuda(logits, labels)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.long
    loss = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
    _check(lib().hvr_ce_rows(_ptr(logits), logits.shape[1], cls_off, ncls, _ptr(labels.contiguous()), logits.shape[0], _ptr(loss),
                             _stream()), 'hvr_ce_rows')
    return loss


def triplet_margin(q, k, anchor_idx, pos_idx, neg_idx, margin, need_grad=True):
    """Stand-in triplet margin loss (see include/hvr_hip.h) -> (out2 = [loss, active triples] f32, dq f32 [Mq,D], dk f32 [Mk,D])."""
    _need_cuda(q, k, anchor_idx, pos_idx, neg_idx)
    assert q.dim() == 2 and k.dim() == 2 and q.shape[1] == k.shape[1] and q.dtype == k.dtype and q.stride(1) == 1 and k.stride(1) == 1
    n = anchor_idx.numel()
    assert n > 0 and pos_idx.numel() == n and neg_idx.numel() == n and anchor_idx.dtype == torch.long
    D = q.shape[1]
    out2 = torch.empty(2, dtype=torch.float32, device=q.device)
    dq = torch.empty((q.shape[0], D), dtype=torch.float32, device=q.device) if need_grad else None
    dk = torch.empty((k.shape[0], D), dtype=torch.float32, device=q.device) if need_grad else None
    ws = _workspace(n * 12, q.device, 'triplet')
    _check(lib().hvr_triplet_margin(_ptr(q), q.stride(0), _ptr(k), k.stride(0), D, q.shape[0], k.shape[0], _ptr(anchor_idx.contiguous()),
                                    _ptr(pos_idx.contiguous()), _ptr(neg_idx.contiguous()), n, float(margin), _dt(q), _ptr(ws), n * 12,
                                    _ptr(out2), _ptr(dq), _ptr(dk), _stream()), 'hvr_triplet_margin')
    return out2, dq, dk


def ingest_frame(frame, new_hw, pad_hw, mean, std, to_rgb=False, flip=None):
    """frame uint8 [H, W, 3] (cuda, rows contiguous) -> f32 [1, 3, pad_h, pad_w]: resize + normalise + pad in one kernel.
    flip: None -> hvr_ingest_frame; True / False -> hvr_ingest_frame_flip (the resized image mirrored before the padding)."""
    _need_cuda(frame)
    assert frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3 and frame.stride(2) == 1 and frame.stride(1) == 3
    out = torch.empty((1, 3, int(pad_hw[0]), int(pad_hw[1])), dtype=torch.float32, device=frame.device)
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    if flip is not None:
        _check(lib().hvr_ingest_frame_flip(_ptr(frame), frame.shape[0], frame.shape[1], frame.stride(0), _ptr(out), int(new_hw[0]), int(new_hw[1]),
                                           int(pad_hw[0]), int(pad_hw[1]), ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p),
                                           int(bool(to_rgb)), int(bool(flip)), _stream()), 'hvr_ingest_frame_flip')
        return out
    _check(lib().hvr_ingest_frame(_ptr(frame), frame.shape[0], frame.shape[1], frame.stride(0), _ptr(out), int(new_hw[0]), int(new_hw[1]),
                                  int(pad_hw[0]), int(pad_hw[1]), ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p),
                                  int(bool(to_rgb)), _stream()), 'hvr_ingest_frame')
    return out


def _aug_arrays(img_w, scale_factor, flip):
    """host arrays (img_w, scale_factor, flip) of the A augmentations for the hvr_*_aug_* calls"""
    A = len(img_w)
    assert A == len(scale_factor) == len(flip) and A > 0
    w = (ctypes.c_float * A)(*[float(v) for v in img_w])
    s = (ctypes.c_float * A)(*[float(v) for v in scale_factor])
    f = (ctypes.c_int32 * A)(*[int(bool(v)) for v in flip])
    return A, w, s, f, (ctypes.cast(w, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), ctypes.cast(f, ctypes.c_void_p))


def merge_aug_proposals(proposals, counts, img_w, scale_factor, flip, nms_thr, max_num):
    """proposals [A,T,mx,5] f32, counts [A,T] int32 (device) + the augmentations' (img_w, scale_factor, flip) host lists ->
    (merged [T,max_num,5] in original-image coordinates, rows behind the count zeroed; merged_counts [T] int32), device tensors."""
    _need_cuda(proposals, counts)
    assert proposals.dtype == torch.float32 and counts.dtype == torch.int32 and proposals.dim() == 4 and proposals.shape[3] == 5
    A, T, mx = (int(v) for v in proposals.shape[:3])
    A_, w, s, f, ptrs = _aug_arrays(img_w, scale_factor, flip)
    assert A_ == A and tuple(counts.shape) == (A, T)
    if A * mx > 8192:
        raise HvrError('hvr_merge_aug_proposals supports A * mx <= 8192, got %d x %d' % (A, mx))
    proposals, counts = proposals.contiguous(), counts.contiguous()
    merged = torch.empty((T, int(max_num), 5), dtype=torch.float32, device=proposals.device)
    mcounts = torch.empty(T, dtype=torch.int32, device=proposals.device)
    ws = _workspace(lib().hvr_merge_aug_proposals_workspace_bytes(A, T, mx), proposals.device, 'tta_merge')
    with _span('merge_aug_proposals', float(proposals.numel() * 4)):
        _check(lib().hvr_merge_aug_proposals(_ptr(proposals), _ptr(counts), A, T, mx, ptrs[0], ptrs[1], ptrs[2], float(nms_thr), int(max_num),
                                             _ptr(merged), _ptr(mcounts), _ptr(ws), ws.numel(), _stream()), 'hvr_merge_aug_proposals')
    return merged, mcounts


def map_aug_rois(merged, img_w, scale_factor, flip):
    """merged [T,max_num,5] (original-image coordinates) -> rois [A, T * max_num, 5] = (frame index, box in augmentation a's coordinates)."""
    _need_cuda(merged)
    assert merged.dtype == torch.float32 and merged.dim() == 3 and merged.shape[2] == 5
    T, mx = int(merged.shape[0]), int(merged.shape[1])
    A, w, s, f, ptrs = _aug_arrays(img_w, scale_factor, flip)
    rois = torch.empty((A, T * mx, 5), dtype=torch.float32, device=merged.device)
    with _span('map_aug_rois', float(rois.numel() * 4)):
        _check(lib().hvr_map_aug_rois(_ptr(merged.contiguous()), A, T, mx, ptrs[0], ptrs[1], ptrs[2], _ptr(rois), _stream()), 'hvr_map_aug_rois')
    return rois


def merge_aug_dets(boxes, scores, img_w, scale_factor, flip):
    """boxes [A,R,4] (each augmentation's own coordinates), scores [A,R,ncls] f32 -> (merged boxes [R,4] at original scale, merged scores [R,ncls])."""
    _need_cuda(boxes, scores)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[2] == 4 and scores.dim() == 3
    A, R, ncls = (int(v) for v in scores.shape)
    A_, w, s, f, ptrs = _aug_arrays(img_w, scale_factor, flip)
    assert A_ == A and tuple(boxes.shape) == (A, R, 4)
    out_b = torch.empty((R, 4), dtype=torch.float32, device=boxes.device)
    out_s = torch.empty((R, ncls), dtype=torch.float32, device=boxes.device)
    with _span('merge_aug_dets', float(boxes.numel() * 4 + scores.numel() * 4)):
        _check(lib().hvr_merge_aug_dets(_ptr(boxes.contiguous()), _ptr(scores.contiguous()), A, R, ncls, ptrs[0], ptrs[1], ptrs[2], _ptr(out_b),
                                        _ptr(out_s), _stream()), 'hvr_merge_aug_dets')
    return out_b, out_s


def mining_argreduce(aff, labels, all_labels):
    """aff f32 [Mq, Mk] (row stride >= Mk), labels int64 [Mq], all_labels int64 [Mk] -> int64 [Mq, 4]:
    (argmax over different-label keys, argmin over same-label keys, top-2 over different-label keys).
    Ties go to the lower index; a row without candidates answers 0 (0, 1 for the pair), a row with one candidate the lowest
    other index as its second pick (0 when Mk == 1).  +-inf affinities are ordinary values.  NaN affinities are unspecified: the
    kernel never selects one, whereas the reference's topk ranks NaN highest."""
    _need_cuda(aff, labels, all_labels)
    assert aff.dtype == torch.float32 and aff.dim() == 2 and aff.stride(1) == 1
    assert labels.dtype == torch.long and all_labels.dtype == torch.long
    Mq, Mk = aff.shape
    assert labels.numel() == Mq and all_labels.numel() == Mk
    out = torch.empty((Mq, 4), dtype=torch.long, device=aff.device)
    _check(lib().hvr_mining_argreduce(_ptr(aff), Mq, Mk, aff.stride(0), _ptr(labels.contiguous()), _ptr(all_labels.contiguous()), _ptr(out),
                                      _stream()), 'hvr_mining_argreduce')
    return out


def det_loss_sampled(logits, cls_off, reg_off, ncls, labels, label_weights, bbox_targets, bbox_weights, sel_counts, beta=1.0):
    """hvr_det_loss in the OHEM form: weights are zero outside the selected rows, sel_counts int32 [2] their number."""
    _need_cuda(logits, labels, label_weights, bbox_targets, bbox_weights, sel_counts)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.long and sel_counts.dtype == torch.int32
    labels, lw, bt, bw = _loss_operands(labels, label_weights, bbox_targets, bbox_weights, logits.shape[0])
    out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    _check(lib().hvr_det_loss_sampled(_ptr(logits), logits.shape[1], cls_off, reg_off, ncls, _ptr(labels), _ptr(lw), _ptr(bt), _ptr(bw),
                                      logits.shape[0], _ptr(sel_counts), float(beta), _ptr(out3), _ptr(dlogits), _stream()),
           'hvr_det_loss_sampled')
    return out3, dlogits


def roi_align_fwd(feat, rois, out_h, out_w, spatial_scale, sample_num, layout, out=None):
    """layout NCHW: feat [B,C,H,W] -> [K,C,oh,ow]; NHWC: feat [B,H,W,C] -> [K,oh,ow,C] (physical shapes).
    out: a contiguous tensor of that shape and feat's dtype to write into (not for split-half maps)."""
    _need_cuda(feat, rois)
    if feat.dtype == SPLIT:   # interpolated in f32, handed back in the split format
        assert out is None
        return cast(roi_align_fwd(cast(feat, torch.float32), rois, out_h, out_w, spatial_scale, sample_num, layout), SPLIT)
    rois = rois.contiguous().float()
    K = rois.shape[0]
    if layout == LAYOUT_NCHW:
        B, C, H, W = feat.shape
        shape = (K, C, out_h, out_w)
    else:
        B, H, W, C = feat.shape
        shape = (K, out_h, out_w, C)
    out = _out(out, shape, feat.dtype, feat.device)
    assert feat.is_contiguous()
    with _span('roi_align', float((feat.numel() + out.numel()) * feat.element_size() + rois.numel() * 4)):
        _check(lib().hvr_roi_align_fwd(_ptr(feat), _ptr(rois), _ptr(out), B, C, H, W, K, out_h, out_w, float(spatial_scale),
                                       int(sample_num), _dt(feat), layout, _stream()), 'hvr_roi_align_fwd')
    return out


def roi_align_bwd(grad_out, rois, feat_shape, spatial_scale, sample_num, layout):
    _need_cuda(grad_out, rois)
    grad_out = grad_out.contiguous().float()
    rois = rois.contiguous().float()
    grad_in = torch.zeros(feat_shape, dtype=torch.float32, device=grad_out.device)
    if layout == LAYOUT_NCHW:
        B, C, H, W = feat_shape
        K, _, PH, PW = grad_out.shape
    else:
        B, H, W, C = feat_shape
        K, PH, PW, _ = grad_out.shape
    _check(lib().hvr_roi_align_bwd(_ptr(grad_out), _ptr(rois), _ptr(grad_in), B, C, H, W, K, PH, PW, float(spatial_scale),
                                   int(sample_num), layout, _stream()), 'hvr_roi_align_bwd')
    return grad_in


def _deform_out_hw(H, W, KH, KW, stride, pad, dil):
    return (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1


def deform_im2col(x, om, KH, KW, stride, pad, dil, deformable_groups, modulated, out=None):
    """The sampler of a (modulated) deformable conv (hvr_deform_im2col): x [B,H,W,Cin] physical NHWC in an operand dtype,
    om [B,OH,OW,ldo] f32 = the raw output of the offset conv (offsets, then mask logits when modulated; ldo may exceed the
    channel count) -> col [B*OH*OW, KH*KW*Cin] of x's dtype, K order [kh][kw][cin].  out: a contiguous tensor of that shape
    to write into."""
    _need_cuda(x, om)
    B, H, W, Cin = x.shape
    OH, OW = _deform_out_hw(H, W, KH, KW, stride, pad, dil)
    assert x.is_contiguous() and om.dtype == torch.float32 and om.is_contiguous() and tuple(om.shape[:3]) == (B, OH, OW), \
        (tuple(x.shape), tuple(om.shape), (B, OH, OW))
    M, K = B * OH * OW, KH * KW * Cin
    out = _out(out, (M, K), x.dtype, x.device)
    # bytes: four corner vectors read and one written per (pixel, tap), the offsets once per pixel
    with _span('deform_im2col', float(5 * M * K * x.element_size() + M * om.shape[3] * 4)):
        _check(lib().hvr_deform_im2col(_ptr(x), _ptr(om), _ptr(out), B, H, W, Cin, KH, KW, int(stride), int(pad), int(dil),
                                       int(deformable_groups), int(bool(modulated)), om.shape[3], _dt(x), _stream()), 'hvr_deform_im2col')
    return out


# Rows of col (output pixels) one sampler + GEMM round of deform_conv2d_nhwc handles, rounded down to whole frames (one frame at
# least): the col scratch stays at about DEFORM_CHUNK_ROWS * 9 * Cin elements however many frames a call carries.  Measured
# (profiles/dcn_bench.txt): 60 frames of 38 x 63 cost the same within 8 % for chunks of 15, 30 or 60 frames and 1.2 - 1.4 x
# as much in chunks of 4; 36 864 rows keep a 15-frame window of that size (35 910 rows) in one chunk.
DEFORM_CHUNK_ROWS = 36864


def deform_conv2d_nhwc(x, om, w, bias, relu, stride, pad, dil, deformable_groups, modulated, out=None, chunk_rows=None):
    """act(deformable conv of x [B,H,W,Cin] with w [Cout,KH,KW,Cin] (the packed layout of conv2d_nhwc) + bias) -> [B,OH,OW,Cout]:
    the sampler (deform_im2col) and the unchanged GEMM, over chunks of whole frames that share one per-stream col scratch.
    A chunk is a set of whole rows of the GEMM's M and the few-row K-sliced route (fewrow_split) is kept off inside, so every
    output row is the same sum whatever the chunking: chunked == unchunked bit for bit.  chunk_rows: None = DEFORM_CHUNK_ROWS,
    0 = one chunk (as few as keep col below the product's 2 GiB operand limit)."""
    _need_cuda(x, om, w, bias)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    OH, OW = _deform_out_hw(H, W, KH, KW, stride, pad, dil)
    out = _out(out, (B, OH, OW, Cout), x.dtype, x.device)
    rows = DEFORM_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    K = KH * KW * Cin
    fpc = B if rows <= 0 else max(1, min(B, rows // (OH * OW)))   # frames per chunk
    fpc = max(1, min(fpc, (2 ** 31 - 1) // (OH * OW * K * x.element_size())))   # (hvr_gemm takes operands below 2 GiB)
    ws = _workspace(fpc * OH * OW * K * x.element_size(), x.device, 'deform_col')
    w2 = w.reshape(Cout, K)
    y2 = out.view(B * OH * OW, Cout)
    with fewrow_split(False):
        for b0 in range(0, B, fpc):
            nb = min(fpc, B - b0)
            m = nb * OH * OW
            col = ws[:m * K * x.element_size()].view(x.dtype).view(m, K)
            deform_im2col(x[b0:b0 + nb], om[b0:b0 + nb], KH, KW, stride, pad, dil, deformable_groups, modulated, out=col)
            gemm(col, w2, bias, relu=relu, out=y2[b0 * OH * OW:b0 * OH * OW + m])
    return out


def _dpool_rows(t, K, what):
    """A per-RoI f32 operand of deform_roi_pool as [K, n] rows with unit column stride (a column slice of a wider GEMM output
    keeps its row stride) -> (tensor, n, row stride)."""
    assert t.dtype == torch.float32 and t.shape[0] == K, (what, t.dtype, tuple(t.shape), K)
    if t.dim() != 2:
        assert t.is_contiguous(), what
        t = t.view(K, -1)
    assert t.shape[1] > 0 and (K <= 1 or (t.stride(1) == 1 and t.stride(0) >= t.shape[1])), (what, tuple(t.shape), t.stride())
    return t, t.shape[1], (t.stride(0) if K > 1 else max(t.stride(0), t.shape[1]))


def deform_roi_pool(feat_nhwc, rois, trans, mask_logit, out_size, out_channels, group_size, part_size, sample_per_part, spatial_scale,
                    trans_std, out=None):
    """Deformable position-sensitive RoI pooling (hvr_deform_roi_pool_fwd; the rule is stated in include/hvr_hip.h): feat_nhwc
    [B,H,W,C] physical NHWC with C = out_channels * group_size^2, rois [K,5] -> [K, P, P, out_channels] of the map's dtype.
    trans: None (no_trans) or f32 [K, ncls*2*ps*ps] / [K, ncls*2, ps, ps] (x offsets then y offsets per class); mask_logit: None or
    f32 [K, P*P] / [K, 1, P, P], the logits whose sigmoid multiplies the result.  Both may be column slices of wider f32 GEMM
    outputs: the row strides are passed on.  out_size: an int or a square pair.  A split-half map is pooled in f32 and handed
    back in the split format, as roi_align_fwd does.  out: a contiguous tensor of the result's shape and dtype to write into.
    Byte model of the span: per output bin up to 4 * sample_per_part^2 corner vectors of out_channels read (fewer where samples share
    cells or are skipped; they hit L2) and one written, plus the rois, offsets and logits once."""
    _need_cuda(feat_nhwc, rois, trans, mask_logit)
    ph, pw = (out_size, out_size) if isinstance(out_size, int) else (int(out_size[0]), int(out_size[1]))
    if feat_nhwc.dtype == SPLIT:
        assert out is None
        return cast(deform_roi_pool(cast(feat_nhwc, torch.float32), rois, trans, mask_logit, (ph, pw), out_channels, group_size, part_size,
                                    sample_per_part, spatial_scale, trans_std), SPLIT)
    rois = rois.contiguous().float()
    assert feat_nhwc.dim() == 4 and feat_nhwc.is_contiguous() and rois.dim() == 2 and rois.shape[1] == 5, (tuple(feat_nhwc.shape), tuple(rois.shape))
    B, H, W, C = feat_nhwc.shape
    K = rois.shape[0]
    part_size = ph if part_size is None else int(part_size[0] if isinstance(part_size, (tuple, list)) else part_size)
    ncls, ldt, ldm = 1, 0, 0
    if trans is not None:
        trans, n, ldt = _dpool_rows(trans, K, 'trans')
        if part_size <= 0 or n % (2 * part_size * part_size):
            raise HvrError('deform_roi_pool: %d offsets per RoI are no multiple of 2 * part_size^2 = %d' % (n, 2 * part_size * part_size))
        ncls = n // (2 * part_size * part_size)
    if mask_logit is not None:
        mask_logit, n, ldm = _dpool_rows(mask_logit, K, 'mask_logit')
        if n != ph * pw:
            raise HvrError('deform_roi_pool: %d mask logits per RoI, out_size is %d x %d' % (n, ph, pw))
    out = _out(out, (K, ph, pw, int(out_channels)), feat_nhwc.dtype, feat_nhwc.device)
    es = feat_nhwc.element_size()
    work = float(K * ph * pw * out_channels * es * (4 * sample_per_part * sample_per_part + 1) + rois.numel() * 4
                 + (0 if trans is None else K * ncls * 2 * part_size * part_size * 4) + (0 if mask_logit is None else K * ph * pw * 4))
    with _span('deform_roi_pool', work):
        _check(lib().hvr_deform_roi_pool_fwd(_ptr(feat_nhwc), _ptr(rois), _ptr(trans), _ptr(mask_logit), _ptr(out), B, H, W, C, K, ph, pw,
                                             int(out_channels), int(group_size), part_size, ncls, int(sample_per_part), float(spatial_scale),
                                             float(trans_std), ldt, ldm, _dt(feat_nhwc), _stream()), 'hvr_deform_roi_pool_fwd')
    return out


def roi_pool_fwd(feat_nhwc, rois, out_h, out_w, spatial_scale, with_argmax=False, out=None):
    """RoI max pooling (hvr_roi_pool_fwd; the rule is stated in include/hvr_hip.h): feat_nhwc [B,H,W,C] physical NHWC, rois [K,5]
    -> out [K,out_h,out_w,C] of the map's dtype, or (out, argmax [K,out_h,out_w,C] int32) with with_argmax.  out: a contiguous
    tensor of the result's shape and dtype to write into (not for split-half maps).  A split-half map is pooled in f32 and handed
    back in the split format, as roi_align_fwd does; the argmax is that of the f32 call.
    Byte model of the span: the map once (a pixel is re-read once per bin that covers it; those reads hit L2), out and the argmax
    written once, the rois once."""
    _need_cuda(feat_nhwc, rois)
    if feat_nhwc.dtype == SPLIT:
        assert out is None
        r = roi_pool_fwd(cast(feat_nhwc, torch.float32), rois, out_h, out_w, spatial_scale, with_argmax)
        return (cast(r[0], SPLIT), r[1]) if with_argmax else cast(r, SPLIT)
    rois = rois.contiguous().float()
    assert feat_nhwc.dim() == 4 and feat_nhwc.is_contiguous() and rois.dim() == 2 and rois.shape[1] == 5, (tuple(feat_nhwc.shape), tuple(rois.shape))
    B, H, W, C = feat_nhwc.shape
    K = rois.shape[0]
    out = _out(out, (K, int(out_h), int(out_w), C), feat_nhwc.dtype, feat_nhwc.device)
    argmax = torch.empty(out.shape, dtype=torch.int32, device=out.device) if with_argmax else None
    work = float((feat_nhwc.numel() + out.numel()) * feat_nhwc.element_size() + (out.numel() * 4 if with_argmax else 0) + rois.numel() * 4)
    with _span('roi_pool', work):
        _check(lib().hvr_roi_pool_fwd(_ptr(feat_nhwc), _ptr(rois), _ptr(out), _ptr(argmax), B, H, W, C, K, int(out_h), int(out_w),
                                      float(spatial_scale), _dt(feat_nhwc), _stream()), 'hvr_roi_pool_fwd')
    return (out, argmax) if with_argmax else out


def roi_pool_bwd(grad_out_nhwc, rois, argmax, feat_shape_nhwc):
    """grad_out [K,PH,PW,C] scattered to the recorded argmax (hvr_roi_pool_bwd) -> grad_in [B,H,W,C] f32, zeroed here."""
    _need_cuda(grad_out_nhwc, rois, argmax)
    grad_out = grad_out_nhwc.contiguous().float()
    rois = rois.contiguous().float()
    B, H, W, C = feat_shape_nhwc
    K, PH, PW, _ = grad_out.shape
    assert argmax.dtype == torch.int32 and argmax.is_contiguous() and tuple(argmax.shape) == (K, PH, PW, C) and rois.shape[0] == K, \
        (argmax.dtype, tuple(argmax.shape), tuple(grad_out.shape), tuple(rois.shape), C)
    grad_in = torch.zeros((B, H, W, C), dtype=torch.float32, device=grad_out.device)
    _check(lib().hvr_roi_pool_bwd(_ptr(grad_out), _ptr(rois), _ptr(argmax), _ptr(grad_in), B, H, W, C, K, PH, PW, _stream()), 'hvr_roi_pool_bwd')
    return grad_in


# ---- the multi-level feature path (csrc/fpn.hip; the rules: include/hvr_hip.h)
def fpn_merge_supported(L, C, dtype):
    """True when hvr_fpn_merge takes L laterals of C channels in the compute format `dtype` (split half: its laterals arrive as f32)."""
    code = HVR_F32 if dtype == SPLIT else DTYPE_CODES.get(dtype)
    return code is not None and bool(lib().hvr_fpn_merge_supported(int(L), int(C), code))


def fpn_merge(laterals, out=None):
    """The FPN top-down pass in one launch (hvr_fpn_merge): laterals [B,H_l,W_l,C] physical NHWC, finest first, each level exactly twice
    the next; f32, bf16 or half (split-half laterals arrive as f32: the lateral convs hand them over with out_f32) -> the list of
    merged maps, lat[l] + the nearest-neighbour upsampled merged map of level l + 1, summed in f32 from the coarsest level inwards
    and rounded once.  The last entry IS the last input.  out: the L - 1 tensors to write into (none may alias an input).
    Byte model of the span: every lateral read once (the coarse re-reads hit L2), every output written once."""
    laterals = list(laterals)
    _need_cuda(*laterals)
    L = len(laterals)
    if L < 1:
        raise HvrError('fpn_merge needs at least one lateral')
    t0 = laterals[0]
    for t in laterals:
        assert t.dim() == 4 and t.is_contiguous(), (tuple(t.shape), t.stride())
        if t.dtype != t0.dtype or t.shape[0] != t0.shape[0] or t.shape[3] != t0.shape[3] or t.device != t0.device:
            raise HvrError('fpn_merge: the laterals differ in dtype, batch, channels or device: %s'
                           % ([(tuple(x.shape), x.dtype) for x in laterals],))
    if t0.dtype == SPLIT:
        raise HvrError('fpn_merge: split-half laterals arrive as f32 (conv2d_nhwc(..., out_f32=True)); merge those and cast once')
    B, _, _, C = t0.shape
    if out is None:
        outs = [torch.empty_like(t) for t in laterals[:-1]]
    else:
        outs = list(out)
        assert len(outs) == L - 1, (len(outs), L)
        for o, t in zip(outs, laterals):
            assert tuple(o.shape) == tuple(t.shape) and o.dtype == t.dtype and o.is_contiguous() and o.device == t.device, (tuple(o.shape), o.dtype)
    lat_p = (ctypes.c_void_p * L)(*[t.data_ptr() for t in laterals])
    out_p = (ctypes.c_void_p * L)(*([o.data_ptr() for o in outs] + [None]))
    Hs = (ctypes.c_int32 * L)(*[t.shape[1] for t in laterals])
    Ws = (ctypes.c_int32 * L)(*[t.shape[2] for t in laterals])
    work = float((sum(t.numel() for t in laterals) + sum(o.numel() for o in outs)) * t0.element_size())
    with _span('fpn_merge', work):
        _check(lib().hvr_fpn_merge(lat_p, out_p, L, B, Hs, Ws, C, _dt(t0), _stream()), 'hvr_fpn_merge')
    return outs + [laterals[-1]]


def roi_levels(rois, num_levels, finest_scale=56):
    """map_roi_levels (single_level.py:55-73) with torch's own expressions: the levels `route='composite'` pools by."""
    scale = torch.sqrt((rois[:, 3] - rois[:, 1] + 1) * (rois[:, 4] - rois[:, 2] + 1))
    lv = torch.floor(torch.log2(scale / finest_scale + 1e-6))
    return torch.nan_to_num(lv, nan=0.0).clamp(min=0, max=num_levels - 1).long()   # (a NaN scale: level 0, the kernel's choice)


def roi_rescale(rois, scale_factor):
    """roi_rescale (single_level.py:75-87), the reference's expressions."""
    cx = (rois[:, 1] + rois[:, 3]) * 0.5
    cy = (rois[:, 2] + rois[:, 4]) * 0.5
    w = rois[:, 3] - rois[:, 1] + 1
    h = rois[:, 4] - rois[:, 2] + 1
    new_w = w * scale_factor
    new_h = h * scale_factor
    x1 = cx - new_w * 0.5 + 0.5
    x2 = cx + new_w * 0.5 - 0.5
    y1 = cy - new_h * 0.5 + 0.5
    y2 = cy + new_h * 0.5 - 0.5
    return torch.stack((rois[:, 0], x1, y1, x2, y2), dim=-1)


ROI_LEVELS_COMPOSITE_SHAPES = frozenset()   # (L, C, K, dtype) at which route=None takes the composite: none measured slower on the one launch


def roi_align_levels(feats, rois, out_size, scales, finest_scale=56, sample_num=2, roi_scale_factor=None, with_levels=False, out=None,
                     route=None):
    """RoIAlign over up to four maps in one launch (hvr_roi_align_levels_fwd): feats [B,H_l,W_l,C] physical NHWC, finest first, rois
    [K,5], scales the levels' spatial scales -> out [K,oh,ow,C] of the maps' dtype, or (out, levels [K] int32) with with_levels.
    Each RoI is pooled on the level its size selects (the rule: include/hvr_hip.h) with the arithmetic of roi_align_fwd on that map.
    roi_scale_factor: the levels come from `rois`, the rescaled boxes (the reference's expressions, roi_rescale) are pooled.
    Split-half maps go through f32 and back, as roi_align_fwd does.  out: a contiguous tensor of the result's shape and dtype.
    route: None / 'kernel' the one launch; 'composite' the reference's loop over the levels on roi_align_fwd, host reads included
    (tests and tools/fpn_bench.py).
    Byte model of the span: the maps once (taps re-read hit L2), out written once, the rois once."""
    feats = list(feats)
    L = len(feats)
    if not 1 <= L <= FPN_MAX_LEVELS:
        raise HvrError('roi_align_levels takes 1 .. %d maps, got %d' % (FPN_MAX_LEVELS, L))
    if len(scales) != L:
        raise HvrError('roi_align_levels: %d maps but %d scales' % (L, len(scales)))
    if route not in (None, 'kernel', 'composite'):
        raise HvrError("roi_align_levels: route %r (None, 'kernel' or 'composite')" % (route,))
    _need_cuda(rois, *feats)
    if feats[0].dtype == SPLIT:
        assert out is None
        r = roi_align_levels([cast(f, torch.float32) for f in feats], rois, out_size, scales, finest_scale, sample_num, roi_scale_factor,
                             with_levels, None, route)
        return (cast(r[0], SPLIT), r[1]) if with_levels else cast(r, SPLIT)
    out_h, out_w = (out_size, out_size) if isinstance(out_size, int) else out_size
    rois = rois.contiguous().float()
    assert rois.dim() == 2 and rois.shape[1] == 5, tuple(rois.shape)
    f0 = feats[0]
    for f in feats:
        assert f.dim() == 4 and f.is_contiguous(), (tuple(f.shape), f.stride())
        if f.dtype != f0.dtype or f.shape[0] != f0.shape[0] or f.shape[3] != f0.shape[3] or f.device != f0.device:
            raise HvrError('roi_align_levels: the maps differ in dtype, batch, channels or device: %s' % ([(tuple(x.shape), x.dtype) for x in feats],))
    B, _, _, C = f0.shape
    K = rois.shape[0]
    pool_rois = rois if roi_scale_factor is None else roi_rescale(rois, roi_scale_factor).contiguous()
    out = _out(out, (K, int(out_h), int(out_w), C), f0.dtype, f0.device)
    if route is None and (L, C, K, f0.dtype) in ROI_LEVELS_COMPOSITE_SHAPES:
        route = 'composite'
    if route == 'composite':
        lv = roi_levels(rois, L, finest_scale)
        out.zero_()
        for i in range(L):
            inds = lv == i
            if inds.any():
                out[inds] = roi_align_fwd(feats[i], pool_rois[inds, :], out_h, out_w, scales[i], sample_num, LAYOUT_NHWC)
        return (out, lv.int()) if with_levels else out
    levels = torch.empty((K,), dtype=torch.int32, device=f0.device) if with_levels else None
    d = RoiLevelsDesc(L=L, B=B, C=C, K=K, PH=int(out_h), PW=int(out_w), sample_num=int(sample_num), dtype=_dt(f0),
                      finest_scale=float(finest_scale), rois=rois.data_ptr(), pool_rois=pool_rois.data_ptr(), out=out.data_ptr(),
                      levels=levels.data_ptr() if levels is not None else None)
    for i, f in enumerate(feats):
        d.feat[i], d.H[i], d.W[i], d.spatial_scale[i] = f.data_ptr(), f.shape[1], f.shape[2], float(scales[i])
    work = float((sum(f.numel() for f in feats) + out.numel()) * f0.element_size() + rois.numel() * 4)
    with _span('roi_align_levels', work):
        _check(lib().hvr_roi_align_levels_fwd(ctypes.byref(d), _stream()), 'hvr_roi_align_levels_fwd')
    return (out, levels) if with_levels else out


# ---- global context block (csrc/gcb.hip; the rule: include/hvr_hip.h)
def gcb_supported(C, dtype):
    """True when the context-block kernels take maps of C channels in the compute format `dtype` (C a multiple of 64 up to 2048; split
    half runs the f32 kernels, cast in and out).  Every other shape is refused with HvrError: there is no second path."""
    return bool(lib().hvr_gcb_supported(int(C), DTYPE_CODES[torch.float32 if dtype == SPLIT else dtype]))


def gcb_splits(B, P, C):
    """The runs the pool cuts a frame's P pixels into: a function of the shape only."""
    return int(lib().hvr_gcb_splits(int(B), int(P), int(C)))


def _gcb_map(u, what):
    if u.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise HvrError('%s: a %s map (float32 / bfloat16 / float16; split half goes through context_block)' % (what, u.dtype))
    if u.dim() != 4 or not u.is_contiguous():
        raise HvrError('%s: the map must be a contiguous physical NHWC tensor, got shape %s strides %s' % (what, tuple(u.shape), u.stride()))
    B, H, W, C = u.shape
    if not gcb_supported(C, u.dtype):
        raise HvrError('%s: C=%d is no multiple of 64 up to 2048 (no kernel, no fallback)' % (what, C))
    return B, H * W, C


def _gcb_f32(t, shape, what):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise HvrError('%s must be a contiguous float32 tensor of shape %s, got %s %s' % (what, tuple(shape), t.dtype, tuple(t.shape)))
    return t


def gcb_pool(u, wm=None):
    """One pass over u [B,H,W,C] (bf16 / half / f32): per frame and pixel run an online-softmax partial (max, sum, acc[C]) of the attention
    pool with mask weights wm f32 [C] (None: the average pool) -> the f32 workspace slab hvr_gcb_transform reads (a view of
    native._workspace: valid until the next gcb_pool on this stream)."""
    _need_cuda(u, wm)
    B, P, C = _gcb_map(u, 'gcb_pool')
    if wm is not None:
        _gcb_f32(wm, (C,), 'gcb_pool: wm')
    nbytes = lib().hvr_gcb_workspace_bytes(B, P, C)
    ws = _workspace(nbytes, u.device, 'gcb')
    with _span('gcb_pool', float(B * P * C * u.element_size())):
        _check(lib().hvr_gcb_pool(_ptr(u), _ptr(wm), _ptr(ws), nbytes, B, P, C, _dt(u), _stream()), 'hvr_gcb_pool')
    return ws[:nbytes].view(torch.float32)[:B * gcb_splits(B, P, C) * (C + 4)].view(B, -1, C + 4)


def _gcb_mlp(branch, C, what):
    if branch is None:
        return None, None
    w1, b1, gamma, beta, w2t, b2 = branch
    R = w1.shape[0]
    _gcb_f32(w1, (R, C), what + ' w1'), _gcb_f32(b1, (R,), what + ' b1'), _gcb_f32(gamma, (R,), what + ' gamma')
    _gcb_f32(beta, (R,), what + ' beta'), _gcb_f32(w2t, (R, C), what + ' w2t'), _gcb_f32(b2, (C,), what + ' b2')
    return GcbMlp(*[t.data_ptr() for t in branch]), R


def gcb_transform(partials, P, mul=None, add=None):
    """partials [B,S,C+4] (gcb_pool's, of frames of P pixels) -> (m [B,C] f32 or None, t [B,C] f32 or None): the context of every frame
    through the bottleneck transforms.  mul / add: (w1 [R,C], b1 [R], ln_weight [R], ln_bias [R], w2t [R,C] = W2 transposed, b2 [C]), all
    f32, or None for an absent branch; m = sigmoid(transform_mul(ctx)), t = transform_add(ctx)."""
    _need_cuda(partials)
    if mul is None and add is None:
        raise HvrError('gcb_transform: neither fusion branch given')
    B, S, C4 = partials.shape
    C = C4 - 4
    if partials.dtype != torch.float32 or not partials.is_contiguous() or S != gcb_splits(B, P, C):
        raise HvrError('gcb_transform: partials %s %s are not gcb_pool\'s of %d frames of %d pixels' % (partials.dtype, tuple(partials.shape), B, P))
    sm, Rm = _gcb_mlp(mul, C, 'gcb_transform: mul')
    sa, Ra = _gcb_mlp(add, C, 'gcb_transform: add')
    if Rm is not None and Ra is not None and Rm != Ra:
        raise HvrError('gcb_transform: the branches have %d and %d bottleneck channels' % (Rm, Ra))
    m = torch.empty((B, C), dtype=torch.float32, device=partials.device) if mul is not None else None
    t = torch.empty((B, C), dtype=torch.float32, device=partials.device) if add is not None else None
    with _span('gcb_transform', float(partials.numel() * 4)):
        _check(lib().hvr_gcb_transform(_ptr(partials), partials.numel() * 4, B, P, C, Rm if Rm is not None else Ra,
                                       ctypes.byref(sm) if sm is not None else None, ctypes.byref(sa) if sa is not None else None, _ptr(m), _ptr(t),
                                       _stream()), 'hvr_gcb_transform')
    return m, t


def gcb_apply(u, m=None, t=None, resid=None, relu=False, out=None):
    """y = act(u * m[n,c] + t[n,c] (+ resid)) in f32, rounded once into u's format.  u [B,H,W,C] bf16 / half / f32, m / t f32 [B,C] or None
    (1 / 0), resid like u or None.  out: a contiguous tensor like u; it may BE u (or resid)."""
    _need_cuda(u, m, t, resid, out)
    B, P, C = _gcb_map(u, 'gcb_apply')
    for x, what in ((m, 'm'), (t, 't')):
        if x is not None:
            _gcb_f32(x, (B, C), 'gcb_apply: ' + what)
    for x, what in ((resid, 'resid'), (out, 'out')):
        if x is not None and (x.dtype != u.dtype or tuple(x.shape) != tuple(u.shape) or not x.is_contiguous()):
            raise HvrError('gcb_apply: %s is %s %s, the map %s %s (same format, same shape, contiguous)' % (what, x.dtype, tuple(x.shape), u.dtype, tuple(u.shape)))
    out = torch.empty_like(u) if out is None else out
    with _span('gcb_apply', float((2 + (resid is not None)) * B * P * C * u.element_size())):
        _check(lib().hvr_gcb_apply(_ptr(u), _ptr(m), _ptr(t), _ptr(resid), _ptr(out), B, P, C, int(bool(relu)), _dt(u), _stream()), 'hvr_gcb_apply')
    return out


def context_block(u, packed, resid=None, relu=False, out=None):
    """The whole block on u [B,H,W,C] in a compute format: pool -> transform -> apply (three launches) -> act(u * m + t (+ resid)).
    packed: dict(wm=f32 [C] or None ('avg'), mul=branch or None, add=branch or None) as gcb_transform takes them (ops.ContextBlock.packed).
    Split half goes through f32 and back, as avgpool_nhwc does.  out as in gcb_apply."""
    _need_cuda(u)
    if u.dtype == SPLIT:
        y = context_block(cast(u, torch.float32), packed, None if resid is None else cast(resid, torch.float32), relu)
        y = cast(y, SPLIT)
        if out is not None:
            out.copy_(y)
            return out
        return y
    B, P, C = _gcb_map(u, 'context_block')
    m, t = gcb_transform(gcb_pool(u, packed.get('wm')), P, packed.get('mul'), packed.get('add'))
    return gcb_apply(u, m, t, resid, relu, out)


# ---- group normalisation (csrc/gn.hip; the rule: include/hvr_hip.h)
def group_norm_supported(C, G, dtype):
    """True when the group-norm kernels take maps of C channels in G groups in the compute format `dtype` (C a multiple of 64 from 64 to
    2048, G divides C, C / G in {2, 4, 8, 16, 32, 64}; split half runs the f32 kernels, cast in and out by the caller).  Every other
    shape is refused with HvrError: there is no second path."""
    return bool(lib().hvr_gn_supported(int(C), int(G), DTYPE_CODES[torch.float32 if dtype == SPLIT else dtype]))


def group_norm_splits(B, P, C):
    """The runs the statistics pass cuts a frame's P pixels into: a function of the shape only."""
    return int(lib().hvr_gn_splits(int(B), int(P), int(C)))


def _gn_map(u, what):
    if u.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise HvrError('%s: a %s map (float32 / bfloat16 / float16; a split-half map is normalised in its float32 form)' % (what, u.dtype))
    if u.dim() != 4 or not u.is_contiguous():
        raise HvrError('%s: the map must be a contiguous physical NHWC tensor, got shape %s strides %s' % (what, tuple(u.shape), u.stride()))
    B, H, W, C = u.shape
    return B, H * W, C


def _gn_ws(ws, B, P, C, G, what):
    S = group_norm_splits(B, P, C)
    if ws.dtype != torch.float32 or tuple(ws.shape) != (B, S, G, 4) or not ws.is_contiguous():
        raise HvrError('%s %s %s is not group_norm_stats\' of %d frames of %d pixels in %d groups: float32 %s'
                       % (what, ws.dtype, tuple(ws.shape), B, P, G, (B, S, G, 4)))
    return ws


def group_norm_stats(u, G):
    """One pass over u [B,H,W,C] (bf16 / half / f32): per frame, pixel run and group the centred partial (count, mean, M2, 0) -> ws f32
    [B,S,G,4], S = group_norm_splits(B, H * W, C), which group_norm_apply merges.  A fresh tensor of torch's allocator (a block holds two
    of them at a time: its conv3's and its shortcut's), so the call can be captured in a graph."""
    _need_cuda(u)
    B, P, C = _gn_map(u, 'group_norm_stats')
    G = int(G)
    S = group_norm_splits(B, P, C)
    nbytes = lib().hvr_gn_workspace_bytes(B, P, C, max(G, 1))
    buf = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=u.device)
    with _span('gn_stats', float(B * P * C * u.element_size())):
        _check(lib().hvr_gn_stats(_ptr(u), _ptr(buf), nbytes, B, P, C, G, _dt(u), _stream()), 'hvr_gn_stats')
    return buf[:B * S * G * 16].view(torch.float32).view(B, S, G, 4)


def group_norm_apply(u, ws, gamma, beta, eps, G, resid=None, resid_norm=None, relu=False, out=None):
    """y = act((u - mean[n,g(c)]) * rstd[n,g(c)] * gamma[c] + beta[c] (+ r)) in f32, rounded once into u's format, mean and rstd merged
    from ws = group_norm_stats(u, G).  gamma / beta f32 [C].  r: nothing, resid (a map like u), or -- resid_norm = (ws_r, gamma_r,
    beta_r), ws_r = group_norm_stats(resid, G) -- resid normalised in the same pass.  out: a contiguous tensor like u; it may BE u (or
    resid)."""
    _need_cuda(u, ws, gamma, beta, resid, out)
    B, P, C = _gn_map(u, 'group_norm_apply')
    G = int(G)
    _gn_ws(ws, B, P, C, G, 'group_norm_apply: ws')
    _gcb_f32(gamma, (C,), 'group_norm_apply: gamma'), _gcb_f32(beta, (C,), 'group_norm_apply: beta')
    ws_r = gamma_r = beta_r = None
    if resid_norm is not None:
        if resid is None:
            raise HvrError('group_norm_apply: resid_norm without resid')
        ws_r, gamma_r, beta_r = resid_norm
        _need_cuda(ws_r, gamma_r, beta_r)
        _gn_ws(ws_r, B, P, C, G, 'group_norm_apply: resid_norm ws')
        _gcb_f32(gamma_r, (C,), 'group_norm_apply: resid_norm gamma'), _gcb_f32(beta_r, (C,), 'group_norm_apply: resid_norm beta')
    for x, what in ((resid, 'resid'), (out, 'out')):
        if x is not None and (x.dtype != u.dtype or tuple(x.shape) != tuple(u.shape) or not x.is_contiguous()):
            raise HvrError('group_norm_apply: %s is %s %s, the map %s %s (same format, same shape, contiguous)'
                           % (what, x.dtype, tuple(x.shape), u.dtype, tuple(u.shape)))
    out = torch.empty_like(u) if out is None else out
    moved = (2 + (resid is not None)) * B * P * C * u.element_size() + (1 + (ws_r is not None)) * ws.numel() * 4
    with _span('gn_apply', float(moved)):
        _check(lib().hvr_gn_apply(_ptr(u), _ptr(ws), _ptr(gamma), _ptr(beta), float(eps), _ptr(resid), _ptr(ws_r), _ptr(gamma_r), _ptr(beta_r),
                                  _ptr(out), B, P, C, G, int(bool(relu)), _dt(u), _stream()), 'hvr_gn_apply')
    return out


def group_norm(u, gamma, beta, G, eps, resid=None, resid_norm=None, relu=False, out=None):
    """torch.nn.GroupNorm(G, C, eps) on u [B,H,W,C] (bf16 / half / f32) with the residual add and the ReLU of a block's close: statistics
    plus apply, two launches.  resid_norm = (the shortcut's group_norm_stats, gamma_r, beta_r).  Arguments as group_norm_apply."""
    _need_cuda(u)
    return group_norm_apply(u, group_norm_stats(u, G), gamma, beta, eps, G, resid, resid_norm, relu, out)


# ---- generalized attention core (csrc/gen_attn.hip; the rule: include/hvr_hip.h)
GEN_ATTN_ENERGY_CAP = 256 << 20   # bytes of f32 the composite route holds at a time in the energies and their softmax together (it works through the image rows in chunks)
# (d, heads, H, W, Hk, Wk) at which the committed run of tools/gen_attention_bench.py shows the kernel SLOWER than the composite: the
# automatic route says composite there
GEN_ATTN_COMPOSITE_SHAPES = frozenset()


def gen_attn_supported(d, heads, Hk, Wk, dtype):
    """True when csrc/gen_attn.hip has an instance: d in (16, 32, 64), Hk + Wk <= 512, bf16 or half.  Pure (no GPU)."""
    return dtype in (torch.bfloat16, torch.float16) and bool(lib().hvr_gen_attn_supported(int(d), int(heads), int(Hk), int(Wk), DTYPE_CODES[dtype]))


def gen_attn_tiles():
    """(queries per workgroup, keys per step of the online softmax) of the kernel."""
    return int(lib().hvr_gen_attn_query_tile()), int(lib().hvr_gen_attn_key_block())


def gen_attn_route(d, heads, H, W, Hk, Wk, dtype, channels=None, route=None):
    """'kernel' or 'composite' for a core of this shape; route='kernel' raises where there is no instance.  channels: the width of the q / k / v
    maps when it is not heads * d (zero-padded maps: composite)."""
    ok = gen_attn_supported(d, heads, Hk, Wk, dtype) and (channels is None or channels == heads * d)
    if route == 'kernel' and not ok:
        raise HvrError('gen_attention: no kernel for d=%d heads=%d Hk+Wk=%d %s channels=%s (d in 16 / 32 / 64, Hk + Wk <= 512, bf16 / half, '
                       'maps of heads * d channels)' % (d, heads, Hk + Wk, dtype, channels))
    if route is not None:
        assert route in ('kernel', 'composite'), route
        return route
    return 'kernel' if ok and (d, heads, H, W, Hk, Wk) not in GEN_ATTN_COMPOSITE_SHAPES else 'composite'


def _gen_attention_composite(q, k, v, heads, d, H, W, Hk, Wk, appr_bias, px, py, gx, gy, qk, out):
    """The reference's formulation (generalized_attention.py:240-368) in torch: energies by matmul, softmax, matmul, in f32 on the stored
    operands, over chunks of image rows; one rounding into the map's format.  The chunk is sized so that the energies AND their softmax,
    the two buffers of [B, heads, rows * W, Mk] f32 that are alive together, stay under GEN_ATTN_ENERGY_CAP (a single image row may
    exceed it).  (q + appr_bias) k is ONE matmul, as in the reference; the position terms are added to it in place."""
    B, Mk, Cq = v.shape[0], Hk * Wk, heads * d
    f = lambda t: t.reshape(B, -1, t.shape[-1])[..., :Cq].float().view(B, -1, heads, d)   # noqa: E731
    v4 = f(v).permute(0, 2, 1, 3)                                             # [B,h,Mk,d]
    kT = f(k).permute(0, 2, 3, 1) if k is not None else None                 # [B,h,d,Mk]
    q5 = f(q).view(B, H, W, heads, d).permute(0, 3, 1, 2, 4) if q is not None else None    # [B,h,H,W,d]
    ab = appr_bias.view(1, heads, 1, 1, d) if appr_bias is not None else None
    rows = max(1, GEN_ATTN_ENERGY_CAP // max(1, 2 * B * heads * W * Mk * 4))
    o = out.view(B, H, W, -1)
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        R = y1 - y0
        qr = q5[:, :, y0:y1] if q5 is not None else None
        if qk:
            e = torch.matmul((qr + ab if ab is not None else qr).reshape(B, heads, R * W, d), kT).view(B, heads, R, W, Hk, Wk)
        elif ab is not None:
            e = torch.matmul(ab.reshape(1, heads, 1, d).expand(B, heads, 1, d), kT).view(B, heads, 1, 1, Hk, Wk).expand(B, heads, R, W, Hk, Wk).contiguous()
        else:
            e = torch.zeros((B, heads, R, W, Hk, Wk), dtype=torch.float32, device=v.device)
        if px is not None:
            e += torch.einsum('bhywd,hwkd->bhywk', qr, px.float()).unsqueeze(4)
            e += torch.einsum('bhywd,hykd->bhywk', qr, py[:, y0:y1].float()).unsqueeze(5)
        if gx is not None:
            e += gx.view(1, heads, 1, W, 1, Wk)
            e += gy[:, y0:y1].reshape(1, heads, R, 1, Hk, 1)
        a = torch.softmax(e.view(B, heads, R * W, Mk), 3)
        del e
        o[:, y0:y1, :, :Cq] = torch.matmul(a, v4).permute(0, 2, 1, 3).reshape(B, R, W, Cq).to(out.dtype)
    return out


def gen_attention(q, k, v, heads, d, H, W, Hk, Wk, appr_bias=None, px=None, py=None, gx=None, gy=None, qk=True, channels=None, route=None):
    """The attention core of a GeneralizedAttention block (the rule: include/hvr_hip.h) -> o [B, H * W, cq].  q [B, H * W, cq] or None, k and
    v [B, Hk * Wk, cq] (k or None), contiguous physical NHWC maps of cq >= heads * d channels in bf16 / half / f32, head m in channels
    [m d, (m + 1) d) (channels past heads * d are padding: zeros in, zeros out).  appr_bias f32 [heads * d]; px [heads,W,Wk,d] and
    py [heads,H,Hk,d] in the maps' format; gx [heads,W,Wk] and gy [heads,H,Hk] f32.  qk: the q . k term is present.  A type whose
    energies do not depend on the query ('0010') is called with H = W = 1 and gives the frame's one row.
    route: None picks the kernel where csrc/gen_attn.hip has an instance (and the measured table does not send the shape to the
    composite), 'kernel' raises where it has none, 'composite' is the reference's formulation in torch over chunks of rows."""
    _need_cuda(q, k, v, appr_bias, px, py, gx, gy)
    if v.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise HvrError('gen_attention: %s maps (float32 / bfloat16 / float16; split half runs the f32 form)' % v.dtype)
    B, cq = v.shape[0], v.shape[-1]
    Cq = heads * d if channels is None else channels
    P, Mk = H * W, Hk * Wk
    if Cq != heads * d or cq < Cq:
        raise HvrError('gen_attention: %d heads of %d channels in maps of %d (%s logical)' % (heads, d, cq, channels))
    if (q is None) != (not (qk or px is not None)) or (k is None) != (not (qk or appr_bias is not None)):
        raise HvrError('gen_attention: q is given exactly when the q.k or q.P terms are, k exactly when the q.k term or appr_bias is')
    if (px is None) != (py is None) or (gx is None) != (gy is None) or (k is None and gx is None and px is None):
        raise HvrError('gen_attention: the position tables come in pairs, and at least one energy term is needed')
    for t, n, what in ((q, P, 'q'), (k, Mk, 'k'), (v, Mk, 'v')):
        if t is not None and (t.dtype != v.dtype or t.numel() != B * n * cq or not t.is_contiguous()):
            raise HvrError('gen_attention: %s is %s %s, expected a contiguous %s map of %d x %d x %d' % (what, t.dtype, tuple(t.shape), v.dtype, B, n, cq))
    for t, shape, dt, what in ((appr_bias, (Cq,), torch.float32, 'appr_bias'), (px, (heads, W, Wk, d), v.dtype, 'px'), (py, (heads, H, Hk, d), v.dtype, 'py'),
                               (gx, (heads, W, Wk), torch.float32, 'gx'), (gy, (heads, H, Hk), torch.float32, 'gy')):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise HvrError('gen_attention: %s is %s %s, expected contiguous %s %s' % (what, t.dtype, tuple(t.shape), dt, shape))
    which = gen_attn_route(d, heads, H, W, Hk, Wk, v.dtype, cq, route)
    if which == 'composite':
        out = torch.zeros((B, P, cq), dtype=v.dtype, device=v.device) if cq != Cq else torch.empty((B, P, cq), dtype=v.dtype, device=v.device)
        with _span('gen_attention_composite', 4.0 * B * heads * P * Mk * d):
            return _gen_attention_composite(q, k, v, heads, d, H, W, Hk, Wk, appr_bias, px, py, gx, gy, qk, out)
    out = torch.empty((B, P, cq), dtype=v.dtype, device=v.device)
    desc = _point(GenAttnDesc(B=B, heads=heads, d=d, H=H, W=W, Hk=Hk, Wk=Wk, qk=int(bool(qk)), dtype=_dt(v)),
                  q=q, k=k, v=v, appr_bias=appr_bias, px=px, py=py, gx=gx, gy=gy, o=out)
    with _span('gen_attention', 4.0 * B * heads * P * Mk * d):
        _check(lib().hvr_gen_attn_fwd(ctypes.byref(desc), _stream()), 'hvr_gen_attn_fwd')
    return out


def nms_first(dets, iou_thr, max_keep, ge_semantics=True):
    """The first max_keep survivors (in score order) of greedy NMS: nms(dets, thr)[:max_keep] of rpn_head.py:95-97, as
    ascending input indices.  dets [n,5] f32 cuda."""
    _need_cuda(dets)
    dets = dets.contiguous().float()
    n = dets.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=dets.device)
    keep = torch.empty(n, dtype=torch.long, device=dets.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=dets.device)
    ws = _workspace(lib().hvr_nms_workspace_bytes(n), dets.device, 'nms')
    _check(lib().hvr_nms_first(_ptr(dets), n, float(iou_thr), int(ge_semantics), int(max_keep), _ptr(keep), _ptr(cnt), _ptr(ws),
                               ws.numel(), _stream()), 'hvr_nms_first')
    return keep[:int(cnt.item())]


def nms(dets, iou_thr, ge_semantics=True):
    """dets [n,5] f32 cuda -> int64 indices kept (ascending input order). One D2H of the count."""
    _need_cuda(dets)
    dets = dets.contiguous().float()
    n = dets.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=dets.device)
    keep = torch.empty(n, dtype=torch.long, device=dets.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=dets.device)
    ws = _workspace(lib().hvr_nms_workspace_bytes(n), dets.device, 'nms')
    _check(lib().hvr_nms(_ptr(dets), n, float(iou_thr), int(ge_semantics), _ptr(keep), _ptr(cnt), _ptr(ws), ws.numel(),
                         _stream()), 'hvr_nms')
    return keep[:int(cnt.item())]


def rpn_proposals(cls, reg, base_anchors, anchor_stride, means, stds, img_shape, nms_pre, nms_post, max_num, nms_thr,
                  wh_ratio_clip=16 / 1000):
    """cls [T,H,W,A] f32, reg [T,H,W,4A] f32 (physical NHWC; may be channel slices of one wider contiguous
    [T,H,W,P] tensor) -> (proposals [T,max_num,5], counts [T] int32)."""
    _need_cuda(cls, reg)
    assert cls.dtype == torch.float32 and reg.dtype == torch.float32
    T, H, W, A = cls.shape
    for t, ch in ((cls, A), (reg, 4 * A)):
        assert t.stride(3) == 1 and t.stride(1) == W * t.stride(2) and t.stride(0) == H * W * t.stride(2) and t.stride(2) >= ch
    props = torch.zeros((T, max_num, 5), dtype=torch.float32, device=cls.device)
    counts = torch.zeros(T, dtype=torch.int32, device=cls.device)
    ba = (ctypes.c_float * (A * 4))(*[float(v) for v in base_anchors.reshape(-1).tolist()])
    mm = (ctypes.c_float * 4)(*[float(v) for v in means])
    ss = (ctypes.c_float * 4)(*[float(v) for v in stds])
    d = RpnDesc(cls=cls.data_ptr(), reg=reg.data_ptr(), T=T, H=H, W=W, A=A, anchor_stride=int(anchor_stride),
                base_anchors=ctypes.cast(ba, ctypes.c_void_p), means=ctypes.cast(mm, ctypes.c_void_p),
                stds=ctypes.cast(ss, ctypes.c_void_p), img_h=float(img_shape[0]), img_w=float(img_shape[1]),
                wh_ratio_clip=float(wh_ratio_clip), nms_pre=int(nms_pre), nms_post=int(nms_post), max_num=int(max_num),
                nms_thr=float(nms_thr), proposals=props.data_ptr(), counts=counts.data_ptr(),
                cls_pitch=cls.stride(2), reg_pitch=reg.stride(2))
    ws = _workspace(lib().hvr_rpn_workspace_bytes(T, H, W, A, int(nms_pre)), cls.device, 'rpn')
    with _span('rpn_proposals', float(cls.numel() * 4 + reg.numel() * 4)):
        _check(lib().hvr_rpn_proposals(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), 'hvr_rpn_proposals')
    return props, counts


def _pixel_slice(t, ch, what):
    """A [T,H,W,ch] f32 map with unit channel stride whose pixels lie at one pitch (a channel slice of a wider contiguous conv output
    keeps that output's pitch) -> the pitch in floats."""
    T, H, W, C = t.shape
    assert t.dtype == torch.float32 and C == ch, (what, tuple(t.shape), t.dtype)
    p = t.stride(2)
    assert (C == 1 or t.stride(3) == 1) and p >= C and t.stride(1) == W * p and t.stride(0) == H * W * p, \
        (what, tuple(t.shape), t.stride())
    return p


def ga_mask_offsets(loc=None, loc_filter_thr=0.01, shape=None, w_off=None, ldo=None, keep=None, om=None):
    """The location mask and / or the offsets of GA-RPN's feature adaption in one launch (hvr_ga_mask_offsets).
    loc [T,H,W,1] f32 logits -> keep [T,H,W] uint8 = (sigmoid(loc) >= loc_filter_thr);
    shape [T,H,W,2] f32, w_off [nch,2] f32 (conv_offset.weight) -> om [T,H,W,ldo] f32 (ldo >= nch, default nch; columns nch.. are
    left as they are), the layout deform_im2col reads.  loc / shape may be channel slices of one conv output.  -> (keep, om),
    None for the half that was not asked for."""
    assert loc is not None or shape is not None
    _need_cuda(loc, shape, w_off)
    ref = loc if loc is not None else shape
    T, H, W = ref.shape[:3]
    lp = sp = 1
    if loc is not None:
        lp = _pixel_slice(loc, 1, 'loc')
        keep = _out(keep, (T, H, W), torch.uint8, loc.device)
    nch = 1
    if shape is not None:
        sp = _pixel_slice(shape, 2, 'shape')
        assert tuple(shape.shape[:3]) == (T, H, W) and w_off is not None and w_off.dtype == torch.float32 and w_off.is_contiguous() \
            and w_off.dim() == 2 and w_off.shape[1] == 2, 'w_off is the [nch, 2] f32 weight of the 1x1 offset conv'
        nch = w_off.shape[0]
        ldo = nch if ldo is None else int(ldo)
        om = _out(om, (T, H, W, ldo), torch.float32, shape.device)
    with _span('ga_mask_offsets', float(T * H * W * (4 + 8 + 1 + 4 * nch))):
        _check(lib().hvr_ga_mask_offsets(_ptr(loc), lp, float(loc_filter_thr), _ptr(keep) if loc is not None else None, _ptr(shape), sp,
                                         _ptr(w_off), _ptr(om) if shape is not None else None, ldo or 0, nch, T * H * W, _stream()),
               'hvr_ga_mask_offsets')
    return (keep if loc is not None else None), (om if shape is not None else None)


def ga_loc_mask(loc, loc_filter_thr, out=None):
    """keep [T,H,W] uint8 = (sigmoid(loc [T,H,W,1] f32) >= loc_filter_thr)."""
    return ga_mask_offsets(loc=loc, loc_filter_thr=loc_filter_thr, keep=out)[0]


def ga_offsets(shape, w_off, ldo=None, out=None):
    """om [T,H,W,ldo] f32 = the 1x1, 2-channel, bias-free offset conv of shape [T,H,W,2] f32 with w_off [nch,2]."""
    return ga_mask_offsets(shape=shape, w_off=w_off, ldo=ldo, om=out)[1]


def masked_conv_max_cout():
    """The most output channels masked_conv2d_nhwc has a kernel for."""
    return int(lib().hvr_masked_conv_max_cout())


def masked_conv2d_nhwc(x, w, bias, keep, pad=0, out=None):
    """Conv at the kept pixels only (hvr_masked_conv_fwd): x [B,H,W,Cin] physical NHWC (bf16 / f16 / f32), w [Cout,KH,KW,Cin] of the
    same dtype, bias [Cout] f32 or None, keep [B,H,W] uint8 (one mask per frame) -> out f32: bias + conv at kept pixels, exactly 0 at
    the others.  out: a [B,H,W,ldo] f32 tensor, ldo >= Cout, whose first Cout columns are written (default: a fresh [B,H,W,Cout]).
    Cout above masked_conv_max_cout() or split-half operands raise HvrError (HVR_EUNSUPPORTED)."""
    _need_cuda(x, w, bias, keep)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    assert x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and w.shape[3] == Cin, (tuple(x.shape), tuple(w.shape), x.dtype, w.dtype)
    assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (B, H, W), (tuple(keep.shape), keep.dtype)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout)
    if out is None:
        out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape[:3]) == (B, H, W) and out.shape[3] >= Cout, tuple(out.shape)
    kept_bytes = float(B * H * W * (1 + 4 * Cout) + Cout * KH * KW * Cin * x.element_size())
    with _span('masked_conv', kept_bytes):
        _check(lib().hvr_masked_conv_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(keep), _ptr(out), B, H, W, Cin, Cout, KH, KW, int(pad),
                                         out.shape[3], _dt(x), _stream()), 'hvr_masked_conv_fwd')
    return out


def ga_rpn_proposals(cls, reg, shape, keep, base_square, anchor_stride, anchoring_means, anchoring_stds, target_means, target_stds,
                     img_shape, nms_pre, nms_post, max_num, nms_thr, wh_ratio_clip=16 / 1000):
    """Guided anchors + proposal read-out (hvr_ga_rpn_proposals): cls [T,H,W,1], reg [T,H,W,4], shape [T,H,W,2] f32 (physical NHWC; may
    be channel slices of wider contiguous conv outputs), keep [T,H,W] uint8 from ga_mask_offsets, base_square [4] (the grid anchor of
    AnchorGenerator(base_size, [octave_base_scale], [1.0])) -> (proposals [T,max_num,5] in score order, counts [T] int32)."""
    _need_cuda(cls, reg, shape, keep)
    T, H, W = cls.shape[:3]
    cp, rp, sp = _pixel_slice(cls, 1, 'cls'), _pixel_slice(reg, 4, 'reg'), _pixel_slice(shape, 2, 'shape')
    assert tuple(reg.shape[:3]) == (T, H, W) and tuple(shape.shape[:3]) == (T, H, W)
    assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (T, H, W), (tuple(keep.shape), keep.dtype)
    props = torch.zeros((T, max_num, 5), dtype=torch.float32, device=cls.device)
    counts = torch.zeros(T, dtype=torch.int32, device=cls.device)

    def f4(v):
        v = v.reshape(-1).tolist() if hasattr(v, 'reshape') else list(v)
        assert len(v) == 4
        return (ctypes.c_float * 4)(*[float(e) for e in v])
    hold = [f4(base_square), f4(anchoring_means), f4(anchoring_stds), f4(target_means), f4(target_stds)]
    hp = [ctypes.cast(h, ctypes.c_void_p) for h in hold]
    d = GaRpnDesc(cls=cls.data_ptr(), reg=reg.data_ptr(), shape=shape.data_ptr(), keep=keep.data_ptr(), T=T, H=H, W=W,
                  anchor_stride=int(anchor_stride), cls_pitch=cp, reg_pitch=rp, shape_pitch=sp, base_square=hp[0], anchoring_means=hp[1],
                  anchoring_stds=hp[2], target_means=hp[3], target_stds=hp[4], img_h=float(img_shape[0]), img_w=float(img_shape[1]),
                  wh_ratio_clip=float(wh_ratio_clip), nms_pre=int(nms_pre), nms_post=int(nms_post), max_num=int(max_num),
                  nms_thr=float(nms_thr), proposals=props.data_ptr(), counts=counts.data_ptr())
    nbytes = lib().hvr_ga_rpn_workspace_bytes(T, H, W, int(nms_pre))
    if not nbytes:
        raise HvrError('ga_rpn_proposals: a %d x %d map is above the 8192 pixels hvr_ga_rpn_proposals selects from' % (H, W))
    ws = _workspace(nbytes, cls.device, 'ga_rpn')
    with _span('ga_rpn_proposals', float(T * H * W * (4 * 7 + 1))):
        _check(lib().hvr_ga_rpn_proposals(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), 'hvr_ga_rpn_proposals')
    return props, counts


def rpn_wide_frames(frames=-1):
    """Calls of rpn_proposals with T <= frames take the chip-wide kernels (same proposals bit for bit); -> previous value."""
    return int(lib().hvr_rpn_wide_frames(int(frames)))


def det_decode(logits, cls_off, reg_off, ncls, rois, means, stds, img_shape, scale_factor, wh_ratio_clip=16 / 1000):
    """logits [R,ld] f32 -> (scores [R,ncls], boxes [R,4])."""
    _need_cuda(logits, rois)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    rois = rois.contiguous().float()
    R = rois.shape[0]
    scores = torch.empty((R, ncls), dtype=torch.float32, device=logits.device)
    boxes = torch.empty((R, 4), dtype=torch.float32, device=logits.device)
    mm = (ctypes.c_float * 4)(*[float(v) for v in means])
    ss = (ctypes.c_float * 4)(*[float(v) for v in stds])
    ih, iw = (float(img_shape[0]), float(img_shape[1])) if img_shape is not None else (0.0, 0.0)
    _check(lib().hvr_det_decode(_ptr(logits), logits.stride(0), cls_off, reg_off, ncls, _ptr(rois), R,
                                ctypes.cast(mm, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), float(wh_ratio_clip),
                                ih, iw, float(scale_factor), _ptr(scores), _ptr(boxes), _stream()), 'hvr_det_decode')
    return scores, boxes


def multiclass_nms(boxes, scores, score_thr, iou_thr, max_num):
    """boxes [R,4], scores [R,ncls] f32 -> (dets [max_num,5], labels [max_num] int64, n int32[1]) device tensors."""
    _need_cuda(boxes, scores)
    R, ncls = scores.shape
    # (the merge kernel writes the count and zeroes the rows behind it: no fill launches in front of it)
    alloc = torch.empty if R > 0 else torch.zeros
    dets = alloc((max_num, 5), dtype=torch.float32, device=boxes.device)
    labels = alloc(max_num, dtype=torch.long, device=boxes.device)
    n_out = alloc(1, dtype=torch.int32, device=boxes.device)
    ws = _workspace(lib().hvr_multiclass_nms_workspace_bytes(R, ncls), boxes.device, 'mcnms')
    _check(lib().hvr_multiclass_nms(_ptr(boxes.contiguous()), _ptr(scores.contiguous()), R, ncls, float(score_thr),
                                    float(iou_thr), int(max_num), _ptr(dets), _ptr(labels), _ptr(n_out), _ptr(ws),
                                    ws.numel(), _stream()), 'hvr_multiclass_nms')
    return dets, labels, n_out


SOFT_NMS_METHODS = {'linear': 1, 'gaussian': 2}     # nms_wrapper.py:87


def _soft_method(method):
    if method not in SOFT_NMS_METHODS:
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))      # nms_wrapper.py:88-90
    return SOFT_NMS_METHODS[method]


def soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3):
    """dets [n,5] f32 cuda (n <= 512) -> (out [n,5]: kept boxes with rescored scores in selection order, inds [n] int64,
    n_out int32[1]) device tensors; rows behind n_out are zero."""
    code = _soft_method(method)
    _need_cuda(dets)
    dets = dets.contiguous().float()
    n = dets.shape[0]
    alloc = torch.empty if n > 0 else torch.zeros
    out = alloc((n, 5), dtype=torch.float32, device=dets.device)
    inds = alloc(n, dtype=torch.long, device=dets.device)
    n_out = alloc(1, dtype=torch.int32, device=dets.device)
    ws = _workspace(lib().hvr_soft_nms_workspace_bytes(n), dets.device, 'softnms1')
    _check(lib().hvr_soft_nms(_ptr(dets), n, float(iou_thr), code, float(sigma), float(min_score), _ptr(out), _ptr(inds), _ptr(n_out),
                              _ptr(ws), ws.numel(), _stream()), 'hvr_soft_nms')
    return out, inds, n_out


def multiclass_soft_nms(boxes, scores, score_thr, iou_thr, max_num, method='linear', sigma=0.5, min_score=1e-3):
    """boxes [R,4] / [P,R,4], scores [R,ncls] / [P,R,ncls] f32 -> (dets [max_num,5], labels [max_num] int64, n int32[1]) device
    tensors, with a leading P on each for the batched form (P problems, one launch pair)."""
    code = _soft_method(method)
    _need_cuda(boxes, scores)
    batched = scores.dim() == 3
    P = scores.shape[0] if batched else 1
    R, ncls = scores.shape[-2:]
    assert boxes.shape[-2:] == (R, 4) and boxes.dim() == scores.dim() and (not batched or boxes.shape[0] == P)
    alloc = torch.empty if R > 0 else torch.zeros
    dets = alloc((P, max_num, 5), dtype=torch.float32, device=boxes.device)
    labels = alloc((P, max_num), dtype=torch.long, device=boxes.device)
    n_out = alloc(P, dtype=torch.int32, device=boxes.device)
    ws = _workspace(lib().hvr_multiclass_soft_nms_workspace_bytes(P, R, ncls), boxes.device, 'mcsoftnms')
    _check(lib().hvr_multiclass_soft_nms(_ptr(boxes.contiguous().float()), _ptr(scores.contiguous().float()), P, R, ncls, float(score_thr),
                                         float(iou_thr), code, float(sigma), float(min_score), int(max_num), _ptr(dets), _ptr(labels),
                                         _ptr(n_out), _ptr(ws), ws.numel(), _stream()), 'hvr_multiclass_soft_nms')
    if batched:
        return dets, labels, n_out
    return dets[0], labels[0], n_out


SEQ_NMS_RESCORE = {'avg': 1, 'max': 2}


def _seq_rescore(rescore):
    if rescore not in SEQ_NMS_RESCORE:
        raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
    return SEQ_NMS_RESCORE[rescore]


def seq_nms(boxes, scores, score_thr, link_iou_thr=0.5, nms_iou_thr=0.3, max_num=300, rescore='avg', phases=None, out=None):
    """Seq-NMS over one video: boxes [F,R,4], scores [F,R,ncls] f32 (the F key frames in time order, R <= 512, padding rows all
    zero scores) -> (dets [F,max_num,5] with the rescored scores, labels [F,max_num] int64, n [F] int32) device tensors; rows
    behind n[t] are zero.  F = 1 equals multiclass_nms(boxes[0], scores[0], score_thr, nms_iou_thr, max_num).
    out = a result triple of these shapes to write into instead of allocating one.
    phases: UNSTABLE measurement hook (tools/seqnms_bench.py), not for products: a mask of 1 link / 2 path / 4 merge -- only those
    kernels run, on the workspace an earlier call with the SAME arguments on this stream filled; any other seq_nms call on the
    stream in between overwrites that workspace and the result is then undefined."""
    code = _seq_rescore(rescore)
    _need_cuda(boxes, scores)
    if scores.dim() != 3 or boxes.dim() != 3 or tuple(boxes.shape) != (scores.shape[0], scores.shape[1], 4):
        raise ValueError('seq_nms takes boxes [F,R,4] and scores [F,R,ncls], got %s and %s' % (tuple(boxes.shape), tuple(scores.shape)))
    F, R, ncls = scores.shape
    alloc = torch.empty if R > 0 else torch.zeros
    dets, labels, n_out = out if out is not None else (alloc((F, max_num, 5), dtype=torch.float32, device=boxes.device),
                                                       alloc((F, max_num), dtype=torch.long, device=boxes.device),
                                                       alloc(F, dtype=torch.int32, device=boxes.device))
    ws = _workspace(lib().hvr_seq_nms_workspace_bytes(F, R, ncls), boxes.device, 'seqnms')
    args = (_ptr(boxes.contiguous().float()), _ptr(scores.contiguous().float()), F, R, ncls, float(score_thr), float(link_iou_thr),
            float(nms_iou_thr), code, int(max_num), _ptr(dets), _ptr(labels), _ptr(n_out), _ptr(ws), ws.numel())
    if phases is None:
        _check(lib().hvr_seq_nms(*args, _stream()), 'hvr_seq_nms')
    else:
        _check(lib().hvr_seq_nms_phases(*args, int(phases), _stream()), 'hvr_seq_nms_phases')
    return dets, labels, n_out


_FRAME_STARTS = {}      # (device, frame counts) -> device int32 [P+1]: a repeated (also a captured) call uploads nothing


def _frame_start(frame_counts, Ftot, device):
    try:
        counts = tuple(int(c) for c in frame_counts)
    except TypeError:
        raise ValueError('frame_counts is a host list of frame counts, got %r' % (frame_counts,))
    if not counts or min(counts) < 1 or sum(counts) != Ftot:
        raise ValueError('frame_counts must hold one count >= 1 per problem and sum to the %d stacked frames, got %s' % (Ftot, list(counts)))
    key = (str(device), counts)
    if key not in _FRAME_STARTS:
        if len(_FRAME_STARTS) >= 256:
            _FRAME_STARTS.clear()
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        _FRAME_STARTS[key] = torch.tensor(starts, dtype=torch.int32, device=device)
    return counts, _FRAME_STARTS[key]


def seq_nms_batched(boxes, scores, frame_counts, score_thr, link_iou_thr=0.5, nms_iou_thr=0.3, max_num=300, rescore='avg', tubes=False,
                    max_tubes=None, out=None):
    """Seq-NMS over P independent problems (one video's key frames for one read-out branch each) in ONE call: boxes [Ftot,R,4],
    scores [Ftot,R,ncls] f32 are the problems' frames stacked, frame_counts the host list of their P frame counts (each >= 1, summing
    to Ftot; ValueError otherwise).  -> (dets [Ftot,max_num,5], labels [Ftot,max_num] int64, n [Ftot] int32), problem by problem
    bit-identical to seq_nms on the slices: nothing crosses a problem boundary.
    tubes=True appends (tube_ids [Ftot,max_num] int32: the problem-local tube of each output row, -1 behind n[t];
    tubes [max_tubes,4] int32: (problem, label, start frame within the problem, length) problem-major then in id order;
    tube_scores [max_tubes] f32; tube_start [P+1] int32, tube_start[P] = the true total).  max_tubes defaults to the candidate bound
    (ncls-1) * Ftot * R; with a smaller one only the first max_tubes rows are written (the rest stays as it was), ids and tube_start
    stay exact.  out = a result tuple of these shapes (3 or 7 tensors) to write into instead of allocating one."""
    code = _seq_rescore(rescore)
    _need_cuda(boxes, scores)
    if scores.dim() != 3 or boxes.dim() != 3 or tuple(boxes.shape) != (scores.shape[0], scores.shape[1], 4):
        raise ValueError('seq_nms takes boxes [F,R,4] and scores [F,R,ncls], got %s and %s' % (tuple(boxes.shape), tuple(scores.shape)))
    Ftot, R, ncls = scores.shape
    counts, starts = _frame_start(frame_counts, Ftot, boxes.device)
    P = len(counts)
    dev = boxes.device
    alloc = torch.empty if R > 0 else torch.zeros
    if max_tubes is None:
        max_tubes = max(ncls - 1, 0) * Ftot * R
    if out is not None:
        if len(out) != (7 if tubes else 3):
            raise ValueError('out holds %d tensors, the call returns %d' % (len(out), 7 if tubes else 3))
        res = tuple(out)
    else:
        res = (alloc((Ftot, max_num, 5), dtype=torch.float32, device=dev), alloc((Ftot, max_num), dtype=torch.long, device=dev),
               alloc(Ftot, dtype=torch.int32, device=dev))
        if tubes:
            ids = alloc((Ftot, max_num), dtype=torch.int32, device=dev) if R > 0 else torch.full((Ftot, max_num), -1, dtype=torch.int32, device=dev)
            res += (ids, alloc((int(max_tubes), 4), dtype=torch.int32, device=dev), alloc(int(max_tubes), dtype=torch.float32, device=dev),
                    alloc(P + 1, dtype=torch.int32, device=dev))
    ws = _workspace(lib().hvr_seq_nms_batched_workspace_bytes(P, Ftot, R, ncls, int(bool(tubes))), dev, 'seqnms')
    tube_ptrs = [_ptr(t) if t.numel() else _ptr(_workspace(16, dev, 'seqnms_none')) for t in res[3:]] if tubes else [None] * 4
    _check(lib().hvr_seq_nms_batched(_ptr(boxes.contiguous().float()), _ptr(scores.contiguous().float()), P, _ptr(starts), Ftot, R, ncls,
                                     float(score_thr), float(link_iou_thr), float(nms_iou_thr), code, int(max_num), _ptr(res[0]), _ptr(res[1]),
                                     _ptr(res[2]), tube_ptrs[0], tube_ptrs[1], tube_ptrs[2], tube_ptrs[3], int(max_tubes) if tubes else 0,
                                     _ptr(ws), ws.numel(), _stream()), 'hvr_seq_nms_batched')
    return res


def readout_nms(boxes, scores, score_thr, nms_cfg, max_num):
    """The multiclass read-out named by an mmdetection nms_cfg (bbox_nms.py:32-34 resolves `type` by name): 'nms' -> multiclass_nms,
    'soft_nms' -> multiclass_soft_nms with the remaining keys (iou_thr, method, sigma, min_score).  Any other type raises."""
    cfg = dict(nms_cfg)
    kind = cfg.pop('type', 'nms')
    if kind == 'nms':
        return multiclass_nms(boxes, scores, score_thr, cfg['iou_thr'], max_num)
    if kind == 'soft_nms':
        return multiclass_soft_nms(boxes, scores, score_thr, cfg.pop('iou_thr'), max_num, **cfg)
    raise NotImplementedError('nms type %r is outside the HVR hot path (nms, soft_nms)' % (kind,))


def cast(x, dtype, scale=None):
    """x in the operand format `dtype`.  Split-half tensors are kept x SPLIT_ACT_SCALE (see the note at as_operand): casting
    into the format applies the factor, casting out of it removes it; `scale` overrides that (as_operand: the weight scale)."""
    _need_cuda(x)
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    if scale is None:
        scale = SPLIT_ACT_SCALE if dtype == SPLIT else (1.0 / SPLIT_ACT_SCALE if x.dtype == SPLIT else 1.0)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _check(lib().hvr_cast_scaled(_ptr(x), _ptr(out), x.numel(), _dt(x), _dt(out), float(scale), _stream()), 'hvr_cast')
    return out


def transpose_pad(x, ldt, out=None):
    """[R, C] -> [C, ldt] with columns R.. zero (the relation's V^T operand)."""
    _need_cuda(x)
    x = x.contiguous()
    R, C = x.shape
    out = _out(out, (C, ldt), x.dtype, x.device)
    _check(lib().hvr_transpose_pad(_ptr(x), _ptr(out), R, C, C, ldt, _dt(x), _stream()), 'hvr_transpose_pad')
    return out


def nchw_to_nhwc(x, dtype=None):
    """[B,C,H,W] contiguous -> physical [B,H,W,C] (optionally casting)."""
    _need_cuda(x)
    x = x.contiguous()
    if dtype == SPLIT or x.dtype == SPLIT:
        assert x.dtype != SPLIT, 'split-half tensors are NHWC only'
        return cast(nchw_to_nhwc(x, torch.float32), SPLIT)
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, C), dtype=dtype or x.dtype, device=x.device)
    _check(lib().hvr_permute_nchw_nhwc(_ptr(x), _ptr(out), B, C, H * W, 1, _dt(x), _dt(out), _stream()), 'hvr_permute')
    return out


def nhwc_to_nchw(x, dtype=None):
    """physical [B,H,W,C] contiguous -> [B,C,H,W] contiguous."""
    _need_cuda(x)
    x = x.contiguous()
    if x.dtype == SPLIT:
        x = cast(x, torch.float32)
    assert dtype != SPLIT, 'split-half tensors are NHWC only'
    B, H, W, C = x.shape
    out = torch.empty((B, C, H, W), dtype=dtype or x.dtype, device=x.device)
    _check(lib().hvr_permute_nchw_nhwc(_ptr(x), _ptr(out), B, C, H * W, 0, _dt(x), _dt(out), _stream()), 'hvr_permute')
    return out
