"""Guided Anchoring RPN head (GA-RPN), inference only.

Mirror of mmdet/models/anchor_heads/guided_anchor_head.py:18-211,271-362 and ga_rpn_head.py:12-127 for one level with sigmoid
objectness: a 3x3 conv + ReLU, a 1x1 location head and a 1x1 anchor-shape head, the feature adaption (a DCN v1 conv whose offsets
are a 1x1 conv of the predicted SHAPE, not of the features), and the objectness / delta heads evaluated only where the location
score passes loc_filter_thr.  `get_bboxes_batched` turns the four maps of all frames of a window into proposals in one device
pipeline: one predicted anchor per kept pixel -> top nms_pre -> delta2bbox -> NMS -> first nms_post -> top max_num.

The location mask is computed ONCE per forward (native.ga_mask_offsets) and kept next to the maps it was made from: the masked
heads and the proposal kernel read the same bytes.  Parameter names are the reference's, so a GA-RPN checkpoint loads strictly.
"""
import numpy as np
import torch
import torch.nn as nn

from . import native
from .backbone import PackedMixin, as_logical, as_nhwc, fold_conv_bn
from .box_ops import AnchorGenerator
from .registry import HEADS


class DeformConvWeights(nn.Module):
    """The parameters of mmdet.ops.DeformConv (dcn/deform_conv.py:190-230: a weight [out, in / groups, k, k] and no bias, the
    constructor asserts `not bias`); the conv itself is native.deform_conv2d_nhwc on the packed weight."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, deformable_groups=1):
        super(DeformConvWeights, self).__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.padding = in_channels, out_channels, kernel_size, padding
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = None
        stdv = 1.0 / np.sqrt(in_channels * kernel_size * kernel_size)
        nn.init.uniform_(self.weight, -stdv, stdv)   # DeformConv.reset_parameters


class FeatureAdaption(nn.Module):
    """guided_anchor_head.py:18-56: conv_offset (1x1, 2 -> deformable_groups * 18, no bias) on the shape map, then DCN v1 + ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size=3, deformable_groups=4):
        super(FeatureAdaption, self).__init__()
        self.conv_offset = nn.Conv2d(2, deformable_groups * kernel_size * kernel_size * 2, 1, bias=False)
        self.conv_adaption = DeformConvWeights(in_channels, out_channels, kernel_size, (kernel_size - 1) // 2, deformable_groups)

    def init_weights(self):
        nn.init.normal_(self.conv_offset.weight, 0, 0.1)
        nn.init.normal_(self.conv_adaption.weight, 0, 0.01)


@HEADS.register_module
class GARPNHead(nn.Module, PackedMixin):

    inference_only = True

    def __init__(self, in_channels, feat_channels=256, octave_base_scale=8, scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0],
                 anchor_strides=[4, 8, 16, 32, 64], anchor_base_sizes=None, anchoring_means=(.0, .0, .0, .0),
                 anchoring_stds=(1.0, 1.0, 1.0, 1.0), target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0),
                 deformable_groups=4, loc_filter_thr=0.01,
                 loss_loc=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_shape=dict(type='BoundedIoULoss', beta=0.2, loss_weight=1.0),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)):
        super(GARPNHead, self).__init__()
        if in_channels != feat_channels:
            raise NotImplementedError('GARPNHead: in_channels (%d) != feat_channels (%d) -- the reference applies conv_loc / conv_shape / the '
                                      'feature adaption, all built for in_channels, to the feat_channels map of rpn_conv '
                                      '(ga_rpn_head.py:28-33), so it only runs when the two are equal' % (in_channels, feat_channels))
        if len(anchor_strides) != 1:
            raise NotImplementedError('GARPNHead: single-level only (anchor_strides=[16]), got %d levels' % len(anchor_strides))
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        if not self.use_sigmoid_cls:
            raise NotImplementedError('GARPNHead: softmax objectness is outside the HVR hot path (use_sigmoid=True)')
        self.in_channels, self.num_classes, self.feat_channels = in_channels, 2, feat_channels
        self.octave_base_scale, self.scales_per_octave = octave_base_scale, scales_per_octave
        self.octave_scales = octave_base_scale * np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)])
        self.octave_ratios = octave_ratios
        self.approxs_per_octave = len(self.octave_scales) * len(octave_ratios)
        self.anchor_strides = anchor_strides
        self.anchor_base_sizes = list(anchor_strides) if anchor_base_sizes is None else anchor_base_sizes
        self.anchoring_means, self.anchoring_stds = anchoring_means, anchoring_stds
        self.target_means, self.target_stds = target_means, target_stds
        self.deformable_groups, self.loc_filter_thr = deformable_groups, loc_filter_thr
        self.approx_generators = [AnchorGenerator(b, self.octave_scales, self.octave_ratios) for b in self.anchor_base_sizes]
        self.square_generators = [AnchorGenerator(b, [self.octave_base_scale], [1.0]) for b in self.anchor_base_sizes]
        self.num_anchors = 1   # one anchor per location
        self.cls_out_channels = self.num_classes - 1
        self.loss_loc_cfg, self.loss_shape_cfg, self.loss_cls_cfg, self.loss_bbox_cfg = loss_loc, loss_shape, loss_cls, loss_bbox
        self.fp16_enabled = False
        for dt in (torch.bfloat16, native.SPLIT, torch.float32):
            if not self._sampler_supported(dt):
                raise NotImplementedError('GARPNHead: %d channels over %d deformable groups is a shape the deformable sampler refuses '
                                          '(hvr_deform_im2col_supported)' % (in_channels, deformable_groups))
        self.rpn_conv = nn.Conv2d(self.in_channels, self.feat_channels, 3, padding=1)
        self.conv_loc = nn.Conv2d(self.in_channels, 1, 1)
        self.conv_shape = nn.Conv2d(self.in_channels, self.num_anchors * 2, 1)
        self.feature_adaption = FeatureAdaption(self.in_channels, self.feat_channels, kernel_size=3, deformable_groups=deformable_groups)
        from .ops import MaskedConv2d
        self.conv_cls = MaskedConv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 1)
        self.conv_reg = MaskedConv2d(self.feat_channels, self.num_anchors * 4, 1)
        self._init_packed()

    def _sampler_supported(self, dtype):
        """hvr_deform_im2col_supported, stated here so that a config is refused where it is built, library or not."""
        C, dg = self.in_channels, self.deformable_groups
        return C > 0 and dg > 0 and C % native.kstep(dtype if dtype != native.SPLIT else torch.float32) == 0 and C % dg == 0 \
            and (C // dg) % 8 == 0

    def init_weights(self):
        """ga_rpn_head.py:24-26, guided_anchor_head.py:187-195, :49-51."""
        nn.init.normal_(self.rpn_conv.weight, 0, 0.01)
        nn.init.constant_(self.rpn_conv.bias, 0)
        for m in (self.conv_cls, self.conv_reg, self.conv_shape):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.conv_loc.weight, 0, 0.01)
        nn.init.constant_(self.conv_loc.bias, float(-np.log((1 - 0.01) / 0.01)))   # bias_init_with_prob(0.01)
        self.feature_adaption.init_weights()
        self._drop_packed()

    def _pack(self, dtype):
        C = self.feat_channels
        dev = self.rpn_conv.weight.device
        wl, bl = fold_conv_bn(self.conv_loc, None, torch.float32)
        wsh, bsh = fold_conv_bn(self.conv_shape, None, torch.float32)
        # location and shape share one GEMM: row 0 the location logit, rows 1..2 the shape deltas, padded to a multiple of 4
        wls = torch.zeros((4, 1, 1, C), dtype=torch.float32, device=dev)
        bls = torch.zeros(4, dtype=torch.float32, device=dev)
        wls[0:1], wls[1:3], bls[0:1], bls[1:3] = wl, wsh, bl, bsh
        # objectness and deltas share one masked conv: row 0 the score, rows 1..4 the deltas; no split-half kernel: the f32 form
        hd = torch.float32 if dtype == native.SPLIT else dtype
        wc, bc = fold_conv_bn(self.conv_cls, None, torch.float32)
        wr, br = fold_conv_bn(self.conv_reg, None, torch.float32)
        wh = torch.cat([wc, wr], 0).contiguous().to(hd)
        bh = torch.cat([bc, br], 0).contiguous()
        return dict(conv=fold_conv_bn(self.rpn_conv, None, dtype), locshape=(native.as_operand(wls, dtype), bls),
                    off=self.feature_adaption.conv_offset.weight.detach().float().reshape(-1, 2).contiguous(),
                    adapt=fold_conv_bn(self.feature_adaption.conv_adaption, None, dtype), heads=(wh, bh))

    def forward_single(self, x):
        """x logical [T,C,H,W] -> (cls [T,1,H,W], reg [T,4,H,W], shape [T,2,H,W], loc [T,1,H,W]) f32, physically NHWC slices of two
        fused outputs.  The keep map of this forward stays on the module beside the loc tensor it was made
        from (`_keep_of`), for get_bboxes_batched."""
        if not x.is_cuda:
            raise NotImplementedError('GARPNHead runs on the GPU only (no CPU fallback)')
        p = self.packed(x.device)
        dt = self.compute_dtype
        dg = self.deformable_groups
        y = native.conv2d_nhwc(as_nhwc(x, dt), p['conv'][0], p['conv'][1], relu=True, pad=1)
        ls = native.conv2d_nhwc(y, p['locshape'][0], p['locshape'][1], relu=False, out_f32=True)     # [T,H,W,4] f32: loc, shape x 2, pad
        loc, shape = ls[..., 0:1], ls[..., 1:3]
        keep, om = native.ga_mask_offsets(loc=loc, loc_filter_thr=self.loc_filter_thr, shape=shape, w_off=p['off'])
        z = native.deform_conv2d_nhwc(y, om, p['adapt'][0], p['adapt'][1], True, 1, 1, 1, dg, False)
        if dt == native.SPLIT:
            z = native.cast(z, torch.float32)
        o = native.masked_conv2d_nhwc(z, p['heads'][0], p['heads'][1], keep)                          # [T,H,W,5] f32
        cls, reg = as_logical(o[..., 0:1]), as_logical(o[..., 1:5])
        shape_l, loc_l = as_logical(shape), as_logical(loc)
        self._keep_of = (loc_l, loc_l._version, keep)
        return cls, reg, shape_l, loc_l

    def forward(self, feats):
        outs = [self.forward_single(f) for f in feats]
        return tuple([o[i] for o in outs] for i in range(4))

    def _keep_for(self, loc, loc_n):
        """The mask the masked heads read.  The rule computes it once per forward, so the proposal kernel is handed that very map when `loc`
        IS the tensor the last forward returned (the same object, not written since: the detectors pass the forward's outputs straight
        on).  Any other loc map -- maps prescribed by a caller, a copy -- gets a mask of its own from the same kernel, which on the same
        values gives the same bytes: the fallback is never wrong, only a second launch.  The pair is replaced at the next forward."""
        k = getattr(self, '_keep_of', None)
        if k is not None and k[0] is loc and loc._version == k[1]:
            return k[2]
        return native.ga_loc_mask(loc_n, self.loc_filter_thr)

    @staticmethod
    def _nhwc_f32(t):
        v = t.permute(0, 2, 3, 1)   # physical NHWC view, no copy
        if v.dtype != torch.float32 or (v.shape[3] > 1 and v.stride(3) != 1) or v.stride(1) != v.shape[2] * v.stride(2) \
                or v.stride(0) != v.shape[1] * v.shape[2] * v.stride(2):
            v = v.float().contiguous()
        return v

    def get_bboxes_batched(self, cls_scores, bbox_preds, shape_preds, loc_preds, img_metas, cfg):
        """(proposals [T,max_num,5], counts [T] int32) on the device, no host synchronisation."""
        if len(cls_scores) != 1:
            raise NotImplementedError('GARPNHead: single-level only (anchor_strides=[16])')
        if cfg.get('nms_across_levels', False) or cfg.get('min_bbox_size', 0) > 0:
            raise NotImplementedError('GARPNHead: nms_across_levels / min_bbox_size > 0 are outside the HVR hot path')
        shape0 = tuple(img_metas[0]['img_shape'][:2])
        if any(tuple(m['img_shape'][:2]) != shape0 for m in img_metas):
            raise NotImplementedError('frames of one window share img_shape (one video)')
        cls_n, reg_n, shape_n, loc_n = (self._nhwc_f32(t[0]) for t in (cls_scores, bbox_preds, shape_preds, loc_preds))
        keep = self._keep_for(loc_preds[0], loc_n)
        return native.ga_rpn_proposals(cls_n, reg_n, shape_n, keep, self.square_generators[0].base_anchors[0], self.anchor_strides[0],
                                       self.anchoring_means, self.anchoring_stds, self.target_means, self.target_stds, shape0,
                                       cfg['nms_pre'], cfg['nms_post'], cfg['max_num'], cfg['nms_thr'])

    def get_bboxes(self, cls_scores, bbox_preds, shape_preds, loc_preds, img_metas, cfg, rescale=False):
        """list of [n_i, 5] proposals per frame (guided_anchor_head.py:561-598); one host read of the counts."""
        props, counts = self.get_bboxes_batched(cls_scores, bbox_preds, shape_preds, loc_preds, img_metas, cfg)
        return [props[i, :c] for i, c in enumerate(counts.tolist())]

    # ---- training: not on the HIP path (core/anchor/guided_anchor_target.py, the four losses) ----
    def _inference_only(self, what):
        raise NotImplementedError('GARPNHead.%s: GARPNHead is inference only (the guided-anchor targets and losses are not on the HIP path)' % what)

    def loss(self, *args, **kwargs):
        self._inference_only('loss')

    def loss_train(self, *args, **kwargs):
        self._inference_only('loss_train')

    def forward_train_fused(self, *args, **kwargs):
        self._inference_only('forward_train_fused')

    def forward_train_nhwc(self, *args, **kwargs):
        self._inference_only('forward_train_nhwc')
