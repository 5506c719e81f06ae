"""FPN neck (mmdet/models/necks/fpn.py:10-141), inference only.

The reference's constructor, state-dict keys (`lateral_convs.{i}.conv.{weight,bias}`, `fpn_convs.{i}.conv.{weight,bias}`: the ConvModule
nesting is kept) and level arithmetic.  `forward` is: the lateral 1x1 convs (native.conv2d_nhwc), ONE native.fpn_merge launch for the whole
top-down pass (the reference: an upsample and an add per level), the 3x3 convs, and the extra levels by a strided slice copy
(`max_pool2d(x, 1, stride=2)` is `x[:, :, ::2, ::2]`) or stride-2 convs.  Maps are logical NCHW over physical NHWC, as the backbone
hands them over.  Split half: the laterals come out as f32 (out_f32), are merged in f32, cast once, and the 3x3 convs run in split half.
`conv_cfg`, `norm_cfg` and activations other than None / 'relu' are refused by name.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native
from .backbone import PackedMixin, as_logical, as_nhwc, fold_conv_bn
from .registry import NECKS


class _Conv(nn.Module):
    """The ConvModule of a neck without a norm layer: `.conv` holds the parameters (the reference's state-dict nesting)."""

    def __init__(self, cin, cout, k, stride=1, padding=0):
        super(_Conv, self).__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding)


def kstep_pad(x, cin):
    """x [B,H,W,C] with zero channels appended up to `cin`, the K-step multiple its conv's packed weight was padded to (a copy; widths
    that are K-step multiples -- every width of the reference's configs -- pass through)."""
    return x if x.shape[-1] == cin else F.pad(x, (0, cin - x.shape[-1]))


@NECKS.register_module
class FPN(nn.Module, PackedMixin):

    inference_only = True

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False, extra_convs_on_inputs=True,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, activation=None):
        super(FPN, self).__init__()
        assert isinstance(in_channels, list)
        if conv_cfg is not None:
            raise NotImplementedError('FPN: conv_cfg=%r is not built (plain convolutions are)' % (conv_cfg,))
        if norm_cfg is not None:
            raise NotImplementedError('FPN: norm_cfg=%r is not built (the reference\'s FPN configs carry none)' % (norm_cfg,))
        if activation not in (None, 'relu'):
            raise NotImplementedError('FPN: activation=%r is not built (None or \'relu\')' % (activation,))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_ins, self.num_outs = len(in_channels), num_outs
        self.activation = activation
        self.relu_before_extra_convs = relu_before_extra_convs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.fp16_enabled = False
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            assert num_outs >= self.num_ins - start_level
        else:   # if end_level < inputs, no extra level is allowed
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        self.start_level, self.end_level = start_level, end_level
        self.add_extra_convs, self.extra_convs_on_inputs = add_extra_convs, extra_convs_on_inputs
        if self.backbone_end_level - start_level > native.FPN_MAX_LEVELS:
            raise NotImplementedError('FPN: %d backbone levels, the merge kernel takes %d'
                                      % (self.backbone_end_level - start_level, native.FPN_MAX_LEVELS))
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(_Conv(in_channels[i], out_channels, 1))
            self.fpn_convs.append(_Conv(out_channels, out_channels, 3, padding=1))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if add_extra_convs and extra_levels >= 1:   # (e.g. RetinaNet)
            for i in range(extra_levels):
                cin = self.in_channels[self.backbone_end_level - 1] if i == 0 and self.extra_convs_on_inputs else out_channels
                self.fpn_convs.append(_Conv(cin, out_channels, 3, stride=2, padding=1))
        self._init_packed()
        for p in self.parameters():
            p.requires_grad = False

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):   # mmcv xavier_init(m, distribution='uniform'): gain 1, bias 0
                nn.init.xavier_uniform_(m.weight, gain=1)
                nn.init.constant_(m.bias, 0)
        self._drop_packed()

    def _pack(self, dtype):
        ks = native.kstep(dtype)

        def one(m):
            w, b = fold_conv_bn(m.conv, None, torch.float32)     # [Cout,KH,KW,Cin] f32
            pad = -w.shape[-1] % ks
            if pad:
                w = F.pad(w, (0, pad))
            return native.as_operand(w, dtype), b
        return dict(lateral=[one(m) for m in self.lateral_convs], fpn=[one(m) for m in self.fpn_convs])

    def _conv(self, x, wb, relu, stride=1, pad=0, out_f32=False):
        return native.conv2d_nhwc(kstep_pad(x, wb[0].shape[-1]), wb[0], wb[1], relu=relu, stride=stride, pad=pad, out_f32=out_f32)

    def forward(self, inputs):
        assert len(inputs) == len(self.in_channels)
        if not inputs[0].is_cuda:
            raise NotImplementedError('FPN runs on the GPU only (no CPU fallback)')
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('FPN is inference only: training through the neck is not on the HIP path')
        dt = self.compute_dtype
        split = dt == native.SPLIT
        p = self.packed(inputs[0].device)
        act = self.activation == 'relu'
        xs = [as_nhwc(x, dt) for x in inputs]
        n = len(self.lateral_convs)
        laterals = [self._conv(xs[i + self.start_level], p['lateral'][i], act, out_f32=split) for i in range(n)]
        merged = native.fpn_merge(laterals)
        if split:
            merged = [native.cast(m, native.SPLIT) for m in merged]
        outs = [self._conv(merged[i], p['fpn'][i], act, pad=1) for i in range(n)]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:   # max_pool2d(outs[-1], 1, stride=2): every other pixel
                for _ in range(self.num_outs - n):
                    outs.append(outs[-1][:, ::2, ::2].contiguous())
            else:
                src = xs[self.backbone_end_level - 1] if self.extra_convs_on_inputs else outs[-1]
                outs.append(self._conv(src, p['fpn'][n], act, stride=2, pad=1))
                for i in range(n + 1, self.num_outs):
                    src = torch.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]
                    outs.append(self._conv(src, p['fpn'][i], act, stride=2, pad=1))
        return tuple(as_logical(o) for o in outs)
