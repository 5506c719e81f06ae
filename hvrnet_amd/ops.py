"""`mmdet.ops` look-alikes backed by libhvr_hip.so.

The reference resolves ops by NAME (`getattr(mmdet.ops, 'RoIAlign')`, roi_extractors/single_level.py:45-52;
`from mmdet.ops import nms`, anchor_heads/rpn_head.py:7; `getattr(nms_wrapper, 'nms')`,
core/post_processing/bbox_nms.py:32-34), so this module exposes the same names with the same call
signatures and error behaviour:
  RoIAlign(out_size, spatial_scale, sample_num=0, use_torchvision=False)   roi_align/roi_align.py:59-87
  roi_align(features, rois, out_size, spatial_scale, sample_num)           roi_align/roi_align.py:56
  RoIPool(out_size, spatial_scale, use_torchvision=False)                  roi_pool/roi_pool.py:53-75
  roi_pool(features, rois, out_size, spatial_scale)                        roi_pool/roi_pool.py:50 (forward and argmax backward)
  nms(dets, iou_thr, device_id=None) -> (dets[inds], inds)                  nms/nms_wrapper.py:8-61
  soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3)      nms/nms_wrapper.py:64-102
  seq_nms(boxes, scores, score_thr, link_iou_thr=0.5, nms_iou_thr=0.3, max_num=300, rescore='avg', *, frame_counts=None, tubes=False)   (no reference counterpart:
                                                                           Seq-NMS over one video, specified in DESIGN.md)
  deform_roi_pooling(data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None,
                     sample_per_part=4, trans_std=.0)                      dcn/deform_pool.py:10-79 (inference only)
  DeformRoIPooling / DeformRoIPoolingPack / ModulatedDeformRoIPoolingPack   dcn/deform_pool.py:82-252 (inference only)
  masked_conv2d(features, mask, weight, bias, padding=0, stride=1)          masked_conv/masked_conv.py:15-61 (inference only)
  MaskedConv2d(in_channels, out_channels, kernel_size, ...)                masked_conv/masked_conv.py:64-89
plus `relation(q, k, v, scale)`: the relation core as an autograd Function with a HIP backward (training path).
CPU tensors raise NotImplementedError exactly like the reference's RoIAlign (roi_align.py:27-28);
NMS follows the reference's CPU semantics (`IoU >= thr` suppresses, nms_cpu.cpp:55).
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import native
from .backbone import PackedMixin


def _pad_rows(w, b, mult=4):
    """Weight rows and bias padded with zeros to a multiple of `mult` outputs (the tile engine's N % 4 == 0)."""
    n = w.shape[0]
    npad = (n + mult - 1) // mult * mult
    if npad == n:
        return w.contiguous(), b.contiguous()
    wp = torch.zeros((npad, w.shape[1]), dtype=w.dtype, device=w.device)
    bp = torch.zeros(npad, dtype=b.dtype, device=b.device)
    wp[:n], bp[:n] = w, b
    return wp, bp


def _channels_last(t):
    """Physical NHWC behind a logical NCHW tensor (ambiguous degenerate shapes count as NCHW)."""
    return t.dim() == 4 and not t.is_contiguous() and t.permute(0, 2, 3, 1).is_contiguous()


class RoIAlignFunction(Function):

    @staticmethod
    def forward(ctx, features, rois, out_size, spatial_scale, sample_num=0):
        out_h, out_w = _pair(out_size)
        assert isinstance(out_h, int) and isinstance(out_w, int)
        if not features.is_cuda:
            raise NotImplementedError
        if rois.dim() != 2 or rois.size(1) != 5:
            raise ValueError('wrong roi size: expected [K, 5], got %s' % (tuple(rois.shape),))
        ctx.spatial_scale, ctx.sample_num = spatial_scale, sample_num
        ctx.save_for_backward(rois)
        ctx.feature_size, ctx.feature_dtype = features.size(), features.dtype
        ctx.nhwc = _channels_last(features)
        if ctx.nhwc:
            out = native.roi_align_fwd(features.permute(0, 2, 3, 1), rois, out_h, out_w, spatial_scale, sample_num,
                                       native.LAYOUT_NHWC)
            return out.permute(0, 3, 1, 2)
        return native.roi_align_fwd(features.contiguous(), rois, out_h, out_w, spatial_scale, sample_num, native.LAYOUT_NCHW)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        rois = ctx.saved_tensors[0]
        assert ctx.feature_size is not None and grad_output.is_cuda
        grad_input = None
        if ctx.needs_input_grad[0]:
            B, C, H, W = ctx.feature_size
            if ctx.nhwc:
                g = native.roi_align_bwd(grad_output.permute(0, 2, 3, 1), rois, (B, H, W, C), ctx.spatial_scale,
                                         ctx.sample_num, native.LAYOUT_NHWC)
                grad_input = native.cast(g, ctx.feature_dtype).permute(0, 3, 1, 2)   # accumulated in f32, handed back in the map's dtype
            else:
                grad_input = native.cast(native.roi_align_bwd(grad_output, rois, (B, C, H, W), ctx.spatial_scale, ctx.sample_num,
                                                              native.LAYOUT_NCHW), ctx.feature_dtype)
        return grad_input, None, None, None, None


roi_align = RoIAlignFunction.apply


class RoIAlign(nn.Module):

    def __init__(self, out_size, spatial_scale, sample_num=0, use_torchvision=False):
        super(RoIAlign, self).__init__()
        if use_torchvision:
            raise NotImplementedError('torchvision is not part of this build')
        self.out_size = _pair(out_size)
        self.spatial_scale = float(spatial_scale)
        self.sample_num = int(sample_num)
        self.use_torchvision = use_torchvision

    def forward(self, features, rois):
        return roi_align(features, rois, self.out_size, self.spatial_scale, self.sample_num)

    def __repr__(self):
        return '%s(out_size=%s, spatial_scale=%s, sample_num=%s, use_torchvision=%s)' % (
            self.__class__.__name__, self.out_size, self.spatial_scale, self.sample_num, self.use_torchvision)


def _pooling_map(data, dtype=None):
    """The physical NHWC map behind `data` [B,C,H,W] (optionally in `dtype`): a channels_last tensor -- logical NCHW over physical
    NHWC, what the window hands over -- is used in place; an NCHW-contiguous one is converted ONCE here (one permute launch, a
    copy of the whole map: callers that pool repeatedly from one map should hand it over channels_last)."""
    if _channels_last(data):
        v = data.permute(0, 2, 3, 1)
        return v if dtype is None or v.dtype == dtype else native.cast(v, dtype)
    return native.nchw_to_nhwc(data.contiguous(), dtype)


class RoIPoolFunction(Function):
    """roi_pool.py:10-47.  features [B,C,H,W] (channels_last: in place; NCHW-contiguous: converted once, _pooling_map), rois [K,5] ->
    the logical [K, C, PH, PW] view of the physical [K, PH, PW, C] result, as RoIAlign hands it to the heads.  The argmax is
    recorded only when the map asks for a gradient; the backward scatters to it (native.roi_pool_bwd) in f32 and hands the
    gradient back in the map's dtype and layout."""

    @staticmethod
    def forward(ctx, features, rois, out_size, spatial_scale):
        out_h, out_w = _pair(out_size)
        assert isinstance(out_h, int) and isinstance(out_w, int)
        if not features.is_cuda:
            raise NotImplementedError
        if rois.dim() != 2 or rois.size(1) != 5:
            raise ValueError('wrong roi size: expected [K, 5], got %s' % (tuple(rois.shape),))
        ctx.feature_size, ctx.feature_dtype = features.size(), features.dtype
        ctx.nhwc = _channels_last(features)
        fmap = _pooling_map(features)
        if features.requires_grad:
            out, argmax = native.roi_pool_fwd(fmap, rois, out_h, out_w, spatial_scale, with_argmax=True)
            ctx.save_for_backward(rois, argmax)
        else:
            out = native.roi_pool_fwd(fmap, rois, out_h, out_w, spatial_scale)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        assert ctx.feature_size is not None and grad_output.is_cuda
        grad_input = None
        if ctx.needs_input_grad[0]:
            rois, argmax = ctx.saved_tensors
            B, C, H, W = ctx.feature_size
            g = native.cast(native.roi_pool_bwd(grad_output.permute(0, 2, 3, 1), rois, argmax, (B, H, W, C)), ctx.feature_dtype)
            grad_input = g.permute(0, 3, 1, 2)   # accumulated in f32, handed back in the map's dtype
            if not ctx.nhwc:
                grad_input = grad_input.contiguous()
        return grad_input, None, None, None


roi_pool = RoIPoolFunction.apply


class RoIPool(nn.Module):

    def __init__(self, out_size, spatial_scale, use_torchvision=False):
        super(RoIPool, self).__init__()
        if use_torchvision:
            raise NotImplementedError('torchvision is not part of this build')
        self.out_size = _pair(out_size)
        self.spatial_scale = float(spatial_scale)
        self.use_torchvision = use_torchvision

    def forward(self, features, rois):
        return roi_pool(features, rois, self.out_size, self.spatial_scale)

    def __repr__(self):
        return '%s(out_size=%s, spatial_scale=%s, use_torchvision=%s)' % (
            self.__class__.__name__, self.out_size, self.spatial_scale, self.use_torchvision)


class DeformRoIPoolingFunction(Function):
    """deform_pool.py:10-79, forward only.  data [B,C,H,W] (channels_last: in place), rois [K,5], offset [K, 2*ncls, ps, ps] (any
    tensor when no_trans) -> the logical [K, out_channels, P, P] view of the physical [K, P, P, out_channels] result."""

    @staticmethod
    def forward(ctx, data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None,
                sample_per_part=4, trans_std=.0):
        out_h, out_w = _pair(out_size)
        assert isinstance(out_h, int) and isinstance(out_w, int)
        assert out_h == out_w
        part_size = out_h if part_size is None else part_size
        assert 0.0 <= trans_std <= 1.0
        if not data.is_cuda:
            raise NotImplementedError
        if rois.dim() != 2 or rois.size(1) != 5:
            raise ValueError('wrong roi size: expected [K, 5], got %s' % (tuple(rois.shape),))
        trans = None
        if not no_trans:
            trans = offset if offset.dtype == torch.float32 else native.cast(offset.contiguous(), torch.float32)
        out = native.deform_roi_pool(_pooling_map(data), rois, trans, None, out_h, out_channels, group_size, part_size,
                                     sample_per_part, spatial_scale, trans_std)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        raise NotImplementedError('inference only')


deform_roi_pooling = DeformRoIPoolingFunction.apply


class DeformRoIPooling(nn.Module):

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0):
        super(DeformRoIPooling, self).__init__()
        self.spatial_scale = spatial_scale
        self.out_size = _pair(out_size)
        self.out_channels = out_channels
        self.no_trans = no_trans
        self.group_size = group_size
        self.part_size = out_size if part_size is None else part_size
        self.sample_per_part = sample_per_part
        self.trans_std = trans_std

    def forward(self, data, rois, offset):
        if self.no_trans:
            offset = data.new_empty(0)
        return deform_roi_pooling(data, rois, offset, self.spatial_scale, self.out_size, self.out_channels, self.no_trans,
                                  self.group_size, self.part_size, self.sample_per_part, self.trans_std)


def _fc_chain(num_fcs, in_features, hidden, out_features, sigmoid):
    """deform_pool.py:134-147 / :197-227: Linear (+ ReLU) ... Linear (+ Sigmoid), the last Linear zero-initialised."""
    seq, ic = [], in_features
    for i in range(num_fcs):
        oc = hidden if i < num_fcs - 1 else out_features
        seq.append(nn.Linear(ic, oc))
        ic = oc
        if i < num_fcs - 1:
            seq.append(nn.ReLU(inplace=True))
        elif sigmoid:
            seq.append(nn.Sigmoid())
    fc = nn.Sequential(*seq)
    last = fc[-2] if sigmoid else fc[-1]
    last.weight.data.zero_()
    last.bias.data.zero_()
    return fc


class _DeformRoIPoolingPackBase(DeformRoIPooling, PackedMixin):
    """What the two packs share: the device chain
        pass 1   native.deform_roi_pool without offsets                       -> x [K, P, P, C] (physical)
        layer 0  of offset_fc and mask_fc as ONE native.gemm (weight rows concatenated, ReLU in the epilogue), whenever both
                 chains have a hidden layer; columns permuted at pack time to the (ph, pw, c) order of x's rows
        layers   1 .. on column slices of that result; the last layer of a chain with an f32 output, its rows padded to a
                 multiple of 4 (98 -> 100 offsets, 49 -> 52 logits: the row strides travel to the kernel)
        pass 2   native.deform_roi_pool with the offsets and, modulated, the mask LOGITS: the sigmoid and the product happen
                 inside the kernel
    with no torch elementwise kernel and no host read.  The modules keep the reference's parameters (offset_fc.N.weight ...), so
    its checkpoints load strictly.  A split-half map is pooled in f32 (converted once for both passes)."""

    def _linears(self, name):
        return [m for m in getattr(self, name, ()) if isinstance(m, nn.Linear)]

    def _pack(self, dtype):
        P, C = self.out_size[0], self.out_channels
        p = {}
        chains = {'off': self._linears('offset_fc'), 'mask': self._linears('mask_fc')}

        def hwc(w):   # columns (c, ph, pw) -> (ph, pw, c)
            return w.view(-1, C, P, P).permute(0, 2, 3, 1).reshape(w.shape[0], -1)

        def layer(fc, first, last):
            w, b = fc.weight.detach().float(), fc.bias.detach().float()
            w = hwc(w) if first else w
            w, b = _pad_rows(w, b) if last else (w.contiguous(), b.contiguous())
            return native.as_operand(w, dtype), b

        fused = all(len(c) > 1 for c in chains.values())
        if fused:
            o0, m0 = chains['off'][0], chains['mask'][0]
            p['fused0'] = (native.as_operand(hwc(torch.cat([o0.weight.detach().float(), m0.weight.detach().float()], 0)), dtype),
                           torch.cat([o0.bias.detach().float(), m0.bias.detach().float()], 0).contiguous())
            p['fused_split'] = o0.weight.shape[0]
        for tag, fcs in chains.items():
            p[tag] = [None if fused and i == 0 else layer(fc, i == 0, i == len(fcs) - 1) for i, fc in enumerate(fcs)]
        return p

    @staticmethod
    def _chain(layers, h, start):
        for i in range(start, len(layers)):
            w, b = layers[i]
            last = i == len(layers) - 1
            h = native.gemm(h, w, b, relu=not last, out_f32=last)
        return h

    def _pool(self, fmap, rois, trans, mask_logit):
        ps = self.part_size[0] if isinstance(self.part_size, (tuple, list)) else self.part_size   # (the reference keeps out_size as given)
        return native.deform_roi_pool(fmap, rois, trans, mask_logit, self.out_size, self.out_channels, self.group_size, ps,
                                      self.sample_per_part, self.spatial_scale, self.trans_std)

    def forward(self, data, rois):
        assert data.size(1) == self.out_channels
        if not data.is_cuda:
            raise NotImplementedError
        dt = self.compute_dtype
        fmap = _pooling_map(data, torch.float32 if dt == native.SPLIT else dt)
        x = self._pool(fmap, rois, None, None)
        K, n = rois.shape[0], self.out_size[0] * self.out_size[1]
        if not self.no_trans and K > 0:
            p = self.packed(data.device)
            rows = x.view(K, -1)
            rows = native.cast(rows, dt) if dt == native.SPLIT else rows
            if 'fused0' in p:
                h = native.gemm(rows, p['fused0'][0], p['fused0'][1], relu=True)
                ho, hm = h[:, :p['fused_split']], h[:, p['fused_split']:]
            else:
                ho = hm = rows
            start = 1 if 'fused0' in p else 0
            trans = self._chain(p['off'], ho, start)[:, :2 * n]
            mask_logit = self._chain(p['mask'], hm, start)[:, :n] if p['mask'] else None
            x = self._pool(fmap, rois, trans, mask_logit)
        x = native.cast(x, dt) if dt == native.SPLIT else x
        return x.permute(0, 3, 1, 2)


class DeformRoIPoolingPack(_DeformRoIPoolingPackBase):

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0,
                 num_offset_fcs=3, deform_fc_channels=1024):
        super(DeformRoIPoolingPack, self).__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size,
                                                   sample_per_part, trans_std)
        self.num_offset_fcs = num_offset_fcs
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            n = self.out_size[0] * self.out_size[1]
            self.offset_fc = _fc_chain(num_offset_fcs, n * out_channels, deform_fc_channels, n * 2, sigmoid=False)
        self._init_packed()


class ModulatedDeformRoIPoolingPack(_DeformRoIPoolingPackBase):

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0,
                 num_offset_fcs=3, num_mask_fcs=2, deform_fc_channels=1024):
        super(ModulatedDeformRoIPoolingPack, self).__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size,
                                                            sample_per_part, trans_std)
        self.num_offset_fcs = num_offset_fcs
        self.num_mask_fcs = num_mask_fcs
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            n = self.out_size[0] * self.out_size[1]
            self.offset_fc = _fc_chain(num_offset_fcs, n * out_channels, deform_fc_channels, n * 2, sigmoid=False)
            self.mask_fc = _fc_chain(num_mask_fcs, n * out_channels, deform_fc_channels, n, sigmoid=True)
        self._init_packed()


class ContextBlock(nn.Module, PackedMixin):
    """mmdet/ops/context_block.py:13-104, the global context block of GCNet: the reference's constructor arguments, assertions,
    parameter names and shapes (conv_mask.*, channel_add_conv.{0,1,3}.*, channel_mul_conv.{0,1,3}.*, LayerNorm weights [planes,1,1]), so
    checkpoints load strictly.  GPU forward only, inference only: pool, transform and apply are native.gcb_* (three launches, no
    torch kernel).  conv_mask.bias shifts every logit of a frame alike and cancels in the softmax: it is loaded and not used."""

    def __init__(self, inplanes, ratio, pooling_type='att', fusion_types=('channel_add', )):
        super(ContextBlock, self).__init__()
        assert pooling_type in ['avg', 'att']
        assert isinstance(fusion_types, (list, tuple))
        valid_fusion_types = ['channel_add', 'channel_mul']
        assert all([f in valid_fusion_types for f in fusion_types])
        assert len(fusion_types) > 0, 'at least one fusion should be used'
        self.inplanes, self.ratio, self.planes = inplanes, ratio, int(inplanes * ratio)   # (int() truncates)
        self.pooling_type, self.fusion_types = pooling_type, fusion_types
        if pooling_type == 'att':
            self.conv_mask = nn.Conv2d(inplanes, 1, kernel_size=1)
            self.softmax = nn.Softmax(dim=2)
        else:
            self.avg_pool = nn.AdaptiveAvgPool2d(1)

        def branch():
            return nn.Sequential(nn.Conv2d(self.inplanes, self.planes, kernel_size=1), nn.LayerNorm([self.planes, 1, 1]), nn.ReLU(inplace=True),
                                 nn.Conv2d(self.planes, self.inplanes, kernel_size=1))
        self.channel_add_conv = branch() if 'channel_add' in fusion_types else None
        self.channel_mul_conv = branch() if 'channel_mul' in fusion_types else None
        self.reset_parameters()
        self._init_packed()

    def reset_parameters(self):
        """context_block.py:54-62: kaiming (fan_in, normal, zero bias) on the mask; the LAST conv of each branch zero, so that a fresh block
        adds 0 (channel_add) or scales by sigmoid(0) = 1/2 (channel_mul)."""
        if self.pooling_type == 'att':
            nn.init.kaiming_normal_(self.conv_mask.weight, a=0, mode='fan_in', nonlinearity='relu')
            nn.init.constant_(self.conv_mask.bias, 0)
            self.conv_mask.inited = True
        for seq in (self.channel_add_conv, self.channel_mul_conv):
            if seq is not None:
                nn.init.constant_(seq[-1].weight, 0)
                nn.init.constant_(seq[-1].bias, 0)

    def _pack(self, dtype):
        """f32 in every compute format (include/hvr_hip.h: everything between the map and the apply is f32); W2 transposed."""
        def f32(t, *shape):
            return t.detach().float().reshape(*shape).contiguous()

        def branch(seq):
            if seq is None:
                return None
            C, R = self.inplanes, self.planes
            return (f32(seq[0].weight, R, C), f32(seq[0].bias, R), f32(seq[1].weight, R), f32(seq[1].bias, R),
                    f32(seq[3].weight, C, R).t().contiguous(), f32(seq[3].bias, C))
        return dict(wm=f32(self.conv_mask.weight, self.inplanes) if self.pooling_type == 'att' else None,
                    mul=branch(self.channel_mul_conv), add=branch(self.channel_add_conv))

    def forward_nhwc(self, u, resid=None, relu=False, out=None):
        """u physical NHWC in a compute format -> act(block(u) (+ resid)); a Bottleneck hands in its identity and relu=True."""
        if self.planes < 1:
            raise native.HvrError('ContextBlock: int(%d * %r) = 0 bottleneck channels' % (self.inplanes, self.ratio))
        return native.context_block(u, self.packed(u.device), resid, relu, out)

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('ContextBlock runs on the GPU only (no CPU fallback)')
        from .backbone import as_logical, as_nhwc
        return as_logical(self.forward_nhwc(as_nhwc(x, self.compute_dtype)))   # (in the compute format, as Bottleneck.forward)


class GeneralizedAttention(nn.Module, PackedMixin):
    """mmdet/models/plugins/generalized_attention.py:10-383, the block of 'An Empirical Study of Spatial Attention Mechanisms in Deep
    Networks': the reference's constructor arguments, parameter names, shapes, registration order and initialisation, so checkpoints load
    strictly.  GPU forward only, inference only.  The three projections and the closing conv are native.conv2d_nhwc calls (the key / value
    subsampling x[:, :, ::s, ::s] is the stride of a 1x1 conv; gamma is folded into proj_conv at pack time, the residual rides on its
    epilogue); the attention core is native.gen_attention (csrc/gen_attn.hip, or the torch composite where the kernel has no instance).
    The position tables depend on the weights and on (H, W) only: they are built in f64 on first use and cached per device, compute
    format and (H, W) until the packed weights are dropped -- a new frame size builds new tables, so warm up before a graph capture.
    Refused: spatial_range >= 0 and q_stride > 1 (the reference cannot build or run them) and the four attention types with bit 1 set
    and bit 3 clear (the reference multiplies Py with the TRANSPOSED query map there: generalized_attention.py:308-326)."""
    core_route = None   # the attention core: None = native.gen_attention chooses by shape; 'kernel' / 'composite' force one (tests, tools)

    def __init__(self, in_dim, spatial_range=-1, num_heads=9, position_embedding_dim=-1, position_magnitude=1, kv_stride=2, q_stride=1,
                 attention_type='1111'):
        super(GeneralizedAttention, self).__init__()
        bits = [bool(int(c)) for c in attention_type]
        if len(bits) != 4 or not any(bits):
            raise ValueError('attention_type is four binary digits with at least one set, got %r' % (attention_type,))
        if bits[1] and not bits[3]:
            raise NotImplementedError('attention_type %r (query content x relative position without the geometry bias) does not compute in the '
                                      'reference: it raises for H != W and multiplies Py with the transposed query map for H == W '
                                      '(generalized_attention.py:308-326); there is nothing to reproduce' % (attention_type,))
        if q_stride != 1:
            raise NotImplementedError('q_stride > 1 raises in the reference (the residual add cannot broadcast): not built')
        if spatial_range >= 0:
            raise NotImplementedError('spatial_range >= 0 (the local constraint map) is not built: only -1, attention over every key')
        if kv_stride < 1 or num_heads < 1 or in_dim // num_heads < 1:
            raise ValueError('kv_stride >= 1, num_heads >= 1 and in_dim // num_heads >= 1 are required')
        self.position_embedding_dim = position_embedding_dim if position_embedding_dim > 0 else in_dim
        self.position_magnitude, self.num_heads, self.channel_in, self.spatial_range = position_magnitude, num_heads, in_dim, spatial_range
        self.kv_stride, self.q_stride, self.attention_type = kv_stride, q_stride, bits
        self.qk_embed_dim = self.v_dim = in_dim // num_heads
        out_c = self.qk_embed_dim * num_heads
        if bits[0] or bits[1]:
            self.query_conv = nn.Conv2d(in_dim, out_c, kernel_size=1, bias=False)
        if bits[0] or bits[2]:
            self.key_conv = nn.Conv2d(in_dim, out_c, kernel_size=1, bias=False)
        self.value_conv = nn.Conv2d(in_dim, out_c, kernel_size=1, bias=False)
        if bits[1] or bits[3]:
            if len(np.arange(0, self.position_embedding_dim / 4)) * 2 != self.position_embedding_dim // 2:
                raise ValueError('position_embedding_dim=%d: the embedding has %d entries, the fc %d inputs (a multiple of 4 is needed)'
                                 % (self.position_embedding_dim, len(np.arange(0, self.position_embedding_dim / 4)) * 2, self.position_embedding_dim // 2))
            self.appr_geom_fc_x = nn.Linear(self.position_embedding_dim // 2, out_c, bias=False)
            self.appr_geom_fc_y = nn.Linear(self.position_embedding_dim // 2, out_c, bias=False)
        stdv = 1.0 / np.sqrt(self.qk_embed_dim * 2)
        if bits[2]:
            self.appr_bias = nn.Parameter(-2 * stdv * torch.rand(out_c) + stdv)
        if bits[3]:
            self.geom_bias = nn.Parameter(-2 * stdv * torch.rand(out_c) + stdv)
        self.proj_conv = nn.Conv2d(out_c, in_dim, kernel_size=1, bias=True)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.init_weights()
        self._tables = {}
        self._init_packed()

    def init_weights(self):
        """generalized_attention.py:374-383: kaiming-uniform with a = 1 on fan_in (|w| <= sqrt(3 / fan_in)) for every conv and fc, zero bias."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_uniform_(m.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _drop_packed(self):
        super(GeneralizedAttention, self)._drop_packed()
        self._tables = {}

    @staticmethod
    def _device_dtype(dtype):
        return torch.float32 if dtype == native.SPLIT else dtype   # split half runs the f32 form, cast in and out (as the context block)

    def _pack(self, dtype):
        """The projections with zero rows / columns up to the conv entries' channel multiples (cin: in_dim, cq: heads * d), gamma folded
        into proj_conv's weight and bias, appr_bias in f32."""
        dt = self._device_dtype(dtype)
        mult = 64 if dt in (torch.bfloat16, torch.float16) else 32
        C, Cq = self.channel_in, self.qk_embed_dim * self.num_heads
        cin, cq = -(-C // mult) * mult, -(-Cq // mult) * mult
        dev = self.value_conv.weight.device

        def proj(conv):
            w = torch.zeros((cq, 1, 1, cin), dtype=torch.float32, device=dev)
            w[:Cq, 0, 0, :C] = conv.weight.detach().float().reshape(Cq, C)
            return w.to(dt).contiguous()
        p = dict(cin=cin, cq=cq, v=proj(self.value_conv))
        if hasattr(self, 'query_conv'):
            p['q'] = proj(self.query_conv)
        if hasattr(self, 'key_conv'):
            p['k'] = proj(self.key_conv)
        g = self.gamma.detach().double().reshape(())
        wo = torch.zeros((C, 1, 1, cq), dtype=torch.float64, device=dev)
        wo[:, 0, 0, :Cq] = self.proj_conv.weight.detach().double().reshape(C, Cq) * g
        p['o'] = (wo.float().to(dt).contiguous(), (self.proj_conv.bias.detach().double() * g).float().contiguous())
        if self.attention_type[2]:
            p['ab'] = self.appr_bias.detach().float().contiguous()
        return p

    def position_tables(self, H, W, device, dtype=None):
        """dict(px [heads,W,Wk,d], py [heads,H,Hk,d] in the compute format; gx [heads,W,Wk], gy [heads,H,Hk] f32 = geom_bias . Px / Py) for an
        [H, W] map -- built in f64 (generalized_attention.py:152-194,226-238), cached.  px / py only for a type with bit 1, gx / gy with bit 3."""
        dt = self._device_dtype(self.compute_dtype if dtype is None else dtype)
        key = (str(device), dt, int(H), int(W))
        if key not in self._tables:
            s, heads, d = self.kv_stride, self.num_heads, self.qk_embed_dim
            F = self.position_embedding_dim
            omega = 1000.0 ** ((4.0 / F) * np.arange(0, F / 4, dtype=np.float64))
            t = {}
            for axis, n, fc in (('x', W, self.appr_geom_fc_x), ('y', H, self.appr_geom_fc_y)):
                nk = (n - 1) // s + 1
                diff = (np.arange(n, dtype=np.float64)[:, None] - s * np.arange(nk, dtype=np.float64)[None, :]) * self.position_magnitude
                ang = diff[:, :, None] / omega
                emb = np.concatenate([np.sin(ang), np.cos(ang)], axis=2)                        # [n, nk, F / 2]
                tab = (emb @ fc.weight.detach().double().cpu().numpy().T) / np.sqrt(2.0)        # [n, nk, heads * d]
                tab = tab.reshape(n, nk, heads, d).transpose(2, 0, 1, 3)                        # [heads, n, nk, d]
                if self.attention_type[1]:
                    t['p' + axis] = torch.from_numpy(np.ascontiguousarray(tab)).float().to(device).to(dt).contiguous()
                if self.attention_type[3]:
                    gb = self.geom_bias.detach().double().cpu().numpy().reshape(heads, 1, 1, d)
                    t['g' + axis] = torch.from_numpy(np.ascontiguousarray((tab * gb).sum(3))).float().to(device).contiguous()
            self._tables[key] = t
        return self._tables[key]

    def forward_nhwc(self, h, out=None):
        """h [B,H,W,in_dim] physical NHWC in a compute format -> gamma * proj_conv(attention(h)) + h; out: where it goes (like h)."""
        native._need_cuda(h)
        if h.dtype == native.SPLIT:
            y = native.cast(self._forward_dev(native.cast(h, torch.float32), None), native.SPLIT)
            if out is not None:
                out.copy_(y)
                return out
            return y
        return self._forward_dev(h, out)

    def _forward_dev(self, h, out):
        p = self.packed(h.device)
        B, H, W, C = h.shape
        t0, t1, t2, t3 = self.attention_type
        s, heads, d = self.kv_stride, self.num_heads, self.qk_embed_dim
        Cq, cq = heads * d, p['cq']
        x = h
        if p['cin'] != C:   # (an in_dim the conv entries do not take: zero channels up to their multiple, against zero weight columns)
            x = torch.zeros((B, H, W, p['cin']), dtype=h.dtype, device=h.device)
            x[..., :C] = h
        Hk, Wk = (H - 1) // s + 1, (W - 1) // s + 1
        q = native.conv2d_nhwc(x, p['q']) if (t0 or t1) else None
        k = native.conv2d_nhwc(x, p['k'], stride=s) if (t0 or t2) else None
        v = native.conv2d_nhwc(x, p['v'], stride=s)
        tabs = self.position_tables(H, W, h.device, h.dtype) if (t1 or t3) else {}
        one_row = not (t0 or t1 or t3)   # '0010': the energies do not depend on the query, every pixel of a frame gets the same row
        qh, qw = (1, 1) if one_row else (H, W)
        o = native.gen_attention(q, k, v, heads, d, qh, qw, Hk, Wk, appr_bias=p.get('ab'), px=tabs.get('px'), py=tabs.get('py'), gx=tabs.get('gx'),
                                 gy=tabs.get('gy'), qk=t0, channels=Cq, route=self.core_route)          # [B, qh * qw, cq]
        wo, bo = p['o']
        if not one_row:
            return native.conv2d_nhwc(o.view(B, H, W, cq), wo, bo, resid=h, relu=False, out=out)
        if native.gcb_supported(C, h.dtype):
            # the frame's one row through proj_conv in f32, then y = h + r[n, c]: the context block's apply with m absent
            r = native.conv2d_nhwc(o.view(B, 1, 1, cq), wo, bo, relu=False, out_f32=True).view(B, C)
            return native.gcb_apply(h, None, r, None, False, out)
        return native.conv2d_nhwc(o.view(B, 1, 1, cq).expand(B, H, W, cq).contiguous(), wo, bo, resid=h, relu=False, out=out)

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('GeneralizedAttention runs on the GPU only (no CPU fallback)')
        from .backbone import as_logical, as_nhwc
        return as_logical(self.forward_nhwc(as_nhwc(x, self.compute_dtype)))   # (in the compute format, as Bottleneck.forward)


def masked_conv2d(features, mask, weight, bias, padding=0, stride=1, dtype=None):
    """MaskedConv2dFunction.forward (masked_conv.py:15-53), forward only: features [B,C,H,W], mask [B,H,W] (or [1,H,W] for one frame, as
    the reference asserts; > 0 keeps), weight [Cout,Cin,k,k], bias [Cout] or None -> [B,Cout,H,W] f32 (physically NHWC): bias + conv at
    the kept pixels, exactly 0 at the others.  One mask per frame (the reference takes batch 1).  dtype: the operand format
    (default: bf16 / f16 / f32 features keep theirs).  Up to native.masked_conv_max_cout() outputs run hvr_masked_conv_fwd, which never
    reads the unkept rows; more outputs take the dense conv and zero the unkept pixels."""
    pad_h, pad_w = _pair(padding)
    stride_h, stride_w = _pair(stride)
    if stride_h != 1 or stride_w != 1:
        raise ValueError('Stride could not only be 1 in masked_conv2d currently.')
    if not features.is_cuda:
        raise NotImplementedError('masked_conv2d runs on the GPU only (no CPU fallback)')
    assert mask.dim() == 3 and features.dim() == 4 and mask.size(0) == features.size(0) and features.size()[2:] == mask.size()[1:]
    Cout, Cin, KH, KW = weight.shape
    if KH != KW or KH % 2 == 0 or pad_h != pad_w or pad_h != (KH - 1) // 2:
        raise NotImplementedError('masked_conv2d: odd square kernels padded to the input size only')
    dtype = dtype or (features.dtype if features.dtype in (torch.bfloat16, torch.float16, torch.float32) else torch.float32)
    from .backbone import as_nhwc, as_logical
    keep = (mask > 0).to(torch.uint8).contiguous()
    w = weight.detach().float().permute(0, 2, 3, 1).contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    if Cout <= native.masked_conv_max_cout():
        op = torch.float32 if dtype == native.SPLIT else dtype     # (no split-half kernel: the f32 form)
        x = as_nhwc(features, op)
        return as_logical(native.masked_conv2d_nhwc(x, w.to(op), b, keep, pad=pad_h))
    x = as_nhwc(features, dtype)
    wp, bp = _pad_rows(w.reshape(Cout, -1), b if b is not None else torch.zeros(Cout, device=w.device))
    y = native.conv2d_nhwc(x, native.as_operand(wp.view(-1, KH, KW, Cin), dtype), bp, relu=False, pad=pad_h, out_f32=True)[..., :Cout]
    return as_logical(torch.where(keep.unsqueeze(-1) != 0, y, torch.zeros((), dtype=y.dtype, device=y.device)))   # (not y * keep: 0 * inf is NaN, an unkept pixel is exactly 0)


class MaskedConv2d(nn.Conv2d):
    """masked_conv.py:64-89: an nn.Conv2d whose forward takes a mask.  mask=None is the plain conv (through conv2d_nhwc, like every conv
    here); with a mask the conv is evaluated at the kept pixels only and the others are exactly 0."""

    def forward(self, input, mask=None):
        if not input.is_cuda:
            raise NotImplementedError('MaskedConv2d runs on the GPU only (no CPU fallback)')
        if mask is None:
            if _pair(self.stride) != (1, 1) or _pair(self.dilation) != (1, 1) or self.groups != 1:
                raise NotImplementedError('MaskedConv2d without a mask: stride 1, no dilation, one group')
            from .backbone import as_nhwc, as_logical
            dtype = input.dtype if input.dtype in (torch.bfloat16, torch.float16, torch.float32) else torch.float32
            Cout, Cin, KH, KW = self.weight.shape
            b = self.bias.detach().float() if self.bias is not None else torch.zeros(Cout, device=input.device)
            wp, bp = _pad_rows(self.weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, -1), b)
            y = native.conv2d_nhwc(as_nhwc(input, dtype), native.as_operand(wp.view(-1, KH, KW, Cin), dtype), bp, relu=False,
                                   pad=_pair(self.padding)[0], out_f32=True)
            return as_logical(y[..., :Cout])
        return masked_conv2d(input, mask, self.weight, self.bias, self.padding)


class RelationFunction(Function):
    """o = softmax(scale * q k^T) v with a HIP backward (the reference differentiates torch.bmm / nn.Softmax / torch.mm,
    selsa_bbox_head.py:166-182, through autograd).  Backward = one score pass (probabilities recomputed, not stored),
    one fused softmax-backward kernel and four tile-engine GEMMs:
        dV = P^T dO      dP = dO V^T      dS = scale * P * (dP - rowsum(dO * O))      dQ = dS K      dK = dS^T Q
    K-contiguous operands for the transposed products come from hvr_transpose_pad (zero-padded to the K-step)."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        if not q.is_cuda:
            raise NotImplementedError('the relation core runs on the GPU only (no CPU fallback)')
        o = native.relation_fwd(q.contiguous(), k.contiguous(), v.contiguous(), scale)
        ctx.save_for_backward(q, k, v, o)
        ctx.scale = float(scale)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_o):
        q, k, v, o = ctx.saved_tensors
        q, k, v, go = q.contiguous(), k.contiguous(), v.contiguous(), grad_o.contiguous().to(q.dtype)
        Mq, D = q.shape
        Mk = k.shape[0]
        step = 64 if q.dtype == torch.bfloat16 else 32              # K-step of the tile engine, in elements
        ldq = (Mq + step - 1) // step * step
        P = native.relation_probs(q, k, ctx.scale)                   # [Mq, ldp], padding columns zero
        ldp = P.shape[1]
        if ldp == Mk:
            vp = v
        else:
            vp = v.new_zeros((ldp, D))                               # V with zero rows for the padded keys
            vp[:Mk] = v
        dP = native.gemm(go, vp)                                     # [Mq, ldp]
        dS = native.relation_dscore(P, dP, go, o, ctx.scale)         # [Mq, ldp]
        go_t = native.transpose_pad(go, ldq)                         # [D, ldq]
        dv = native.gemm(native.transpose_pad(P, ldq)[:Mk], go_t)    # P^T dO        -> [Mk, D]
        dq = native.gemm(dS, native.transpose_pad(k, ldp))           # dS K          -> [Mq, D]
        dk = native.gemm(native.transpose_pad(dS, ldq)[:Mk], native.transpose_pad(q, ldq))  # dS^T Q -> [Mk, D]
        return dq, dk, dv, None


relation = RelationFunction.apply


class SigmoidFocalLossFunction(Function):
    """mmdet/ops/sigmoid_focal_loss/sigmoid_focal_loss.py:8-34: the elementwise loss [N, C] of logits [N, C] (f32 / bf16 / half) and
    int64 targets [N] (0 background, c + 1 class c, < 0 nothing), with the kernels' own backward.  The rule: include/hvr_hip.h."""

    @staticmethod
    def forward(ctx, input, target, gamma=2.0, alpha=0.25):
        ctx.save_for_backward(input, target)
        ctx.gamma, ctx.alpha = float(gamma), float(alpha)
        loss = native.sigmoid_focal_loss_fwd(input if input.stride(-1) == 1 else input.contiguous(), target.contiguous(), ctx.gamma, ctx.alpha)
        return loss if input.dtype == torch.float32 else loss.to(input.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        input, target = ctx.saved_tensors
        d_input = native.sigmoid_focal_loss_bwd(input if input.stride(-1) == 1 else input.contiguous(), target.contiguous(),
                                                d_loss.float().contiguous(), ctx.gamma, ctx.alpha)
        return (d_input if input.dtype == torch.float32 else d_input.to(input.dtype)), None, None, None


sigmoid_focal_loss = SigmoidFocalLossFunction.apply


def _rows(t):
    """A 2-D f32 view whose rows are contiguous (any row pitch), or a contiguous copy."""
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1] else t.contiguous()


class RegLossFunction(Function):
    """The elementwise ('none') form of the regression losses (csrc/reg_loss.hip; the rules: include/hvr_hip.h): pred, target f32
    [N, D] -> loss [N, D], with the kernels' own backward (to pred only)."""

    @staticmethod
    def forward(ctx, pred, target, rule, beta, alpha, gamma):
        assert pred.dim() == 2 and pred.shape == target.shape, '%s: pred and target [N, D] of one shape' % rule
        p, t = _rows(pred), target.float().contiguous()
        ctx.save_for_backward(p, t)
        ctx.args = (rule, float(beta), float(alpha), float(gamma))
        return native.reg_loss_fwd(rule, p, t, *ctx.args[1:])

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        p, t = ctx.saved_tensors
        return (native.reg_loss_bwd(ctx.args[0], p, t, d_loss.float().contiguous(), *ctx.args[1:]),) + (None,) * 5


class BoxLossFunction(Function):
    """The elementwise form of the box-pair losses: pred, target f32 [n, 4] -> loss [n] ('iou') / [n, 4] ('bounded_iou')."""

    @staticmethod
    def forward(ctx, pred, target, rule, beta, eps):
        assert pred.dim() == 2 and pred.shape[1] == 4 and pred.shape == target.shape, '%s: pred and target [n, 4]' % rule
        p, t = pred.float().contiguous(), target.float().contiguous()
        ctx.save_for_backward(p, t)
        ctx.args = (rule, float(beta), float(eps))
        return native.box_loss_fwd(rule, p, t, *ctx.args[1:])

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        p, t = ctx.saved_tensors
        return (native.box_loss_bwd(ctx.args[0], p, t, d_loss.float().contiguous(), *ctx.args[1:]),) + (None,) * 4


def smooth_l1_loss(pred, target, beta=1.0):
    """smooth_l1_loss.py:8-18 without the reduction: [N, D]."""
    return RegLossFunction.apply(pred, target, 'smooth_l1', beta, 0.0, 0.0)


def balanced_l1_loss(pred, target, beta=1.0, alpha=0.5, gamma=1.5):
    """balanced_l1_loss.py:9-27 without the reduction: [N, D]."""
    return RegLossFunction.apply(pred, target, 'balanced_l1', beta, alpha, gamma)


def mse_loss(pred, target):
    """F.mse_loss(reduction='none'): [N, D]."""
    return RegLossFunction.apply(pred, target, 'mse', 0.0, 0.0, 0.0)


def iou_loss(pred, target, eps=1e-6):
    """iou_loss.py:9-26 without the reduction: [n]."""
    return BoxLossFunction.apply(pred, target, 'iou', 0.0, eps)


def bounded_iou_loss(pred, target, beta=0.2, eps=1e-3):
    """iou_loss.py:29-63 without the reduction: [n, 4]."""
    return BoxLossFunction.apply(pred, target, 'bounded_iou', beta, eps)


class SigmoidFocalLoss(nn.Module):
    """sigmoid_focal_loss.py:40-54: forward returns loss.sum()."""

    def __init__(self, gamma, alpha):
        super(SigmoidFocalLoss, self).__init__()
        self.gamma, self.alpha = gamma, alpha

    def forward(self, logits, targets):
        assert logits.is_cuda
        return sigmoid_focal_loss(logits, targets, self.gamma, self.alpha).sum()

    def __repr__(self):
        return self.__class__.__name__ + '(gamma={}, alpha={})'.format(self.gamma, self.alpha)


def nms(dets, iou_thr, device_id=None):
    """Same dispatch contract as nms_wrapper.nms: tensor or ndarray in, same type out."""
    if isinstance(dets, torch.Tensor):
        is_numpy = False
        dets_th = dets
    elif isinstance(dets, np.ndarray):
        is_numpy = True
        dets_th = torch.from_numpy(dets).to('cuda:%d' % (device_id or 0))
    else:
        raise TypeError('dets must be either a Tensor or numpy array, but got {}'.format(type(dets)))
    if dets_th.shape[0] == 0:
        inds = dets_th.new_zeros(0, dtype=torch.long)
    else:
        if not dets_th.is_cuda:
            raise NotImplementedError('hvr nms runs on the GPU only (no CPU fallback)')
        inds = native.nms(dets_th, iou_thr, ge_semantics=True)
    if is_numpy:
        inds = inds.cpu().numpy()
    return dets[inds, :], inds


def soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3):
    """nms_wrapper.soft_nms (nms_wrapper.py:64-102) on the device: (new_dets [k,5] = the kept boxes with their rescored scores in
    selection order, inds [k] int64).  At most 512 boxes.  One host read (k); the reference copies the list to numpy and back."""
    if method not in native.SOFT_NMS_METHODS:
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    if not isinstance(dets, torch.Tensor):
        raise TypeError('dets must be a Tensor, but got {}'.format(type(dets)))
    if not dets.is_cuda:
        raise NotImplementedError('hvr soft_nms runs on the GPU only (no CPU fallback)')
    if dets.shape[0] == 0:
        return dets.new_zeros((0, 5)), dets.new_zeros(0, dtype=torch.long)
    out, inds, n = native.soft_nms(dets, iou_thr, method, sigma, min_score)
    k = int(n.item())
    return out[:k].to(dets.dtype), inds[:k]


def seq_nms(boxes, scores, score_thr, link_iou_thr=0.5, nms_iou_thr=0.3, max_num=300, rescore='avg', *, frame_counts=None, tubes=False):
    """Seq-NMS (Han et al. 2016) over the key frames of ONE video on the device: boxes [F,R,4] (class-agnostic), scores [F,R,ncls]
    (column 0 = background), frames in time order -> (dets [F,max_num,5], labels [F,max_num] int64, n [F] int32) device tensors.
    Per class, boxes of adjacent frames link at IoU >= link_iou_thr; the highest-scoring sequence is selected, its boxes rescored
    ('avg': sum / length, 'max': the sequence's best score) and kept, their in-frame overlaps at IoU >= nms_iou_thr dropped, until
    no box with score > score_thr is left; per frame the kept boxes come out as multiclass_nms lists them (class-major, cut to the
    max_num best).  DESIGN.md holds the exact specification; one frame gives per-class greedy NMS.
    frame_counts = [F_0, F_1, ...] (host list summing to F): the frames are those of several independent problems (videos, read-out
    branches) stacked, processed side by side in one call; nothing links across a boundary.  tubes=True appends (tube_ids
    [F,max_num] int32, tubes [n,4] int32 = (problem, label, start frame within the problem, length), tube_scores [n] f32, tube_start
    [P+1] int32): which selected sequence every output row belongs to (native.seq_nms_batched)."""
    if rescore not in native.SEQ_NMS_RESCORE:
        raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
    if not isinstance(boxes, torch.Tensor) or not isinstance(scores, torch.Tensor):
        raise TypeError('boxes and scores must be Tensors, but got {} and {}'.format(type(boxes), type(scores)))
    if not boxes.is_cuda or not scores.is_cuda:
        raise NotImplementedError('hvr seq_nms runs on the GPU only (no CPU fallback)')
    if frame_counts is None and not tubes:
        return native.seq_nms(boxes, scores, score_thr, link_iou_thr, nms_iou_thr, max_num, rescore)
    return native.seq_nms_batched(boxes, scores, [scores.shape[0]] if frame_counts is None else frame_counts, score_thr, link_iou_thr,
                                  nms_iou_thr, max_num, rescore, tubes=tubes)
