"""ResNet-C4 backbone and the res5 shared head, executed by the gfx950 implicit-GEMM kernels.

Host-side mirror of mmdet/models/backbones/resnet.py (Bottleneck 86-266, make_res_layer 269-329,
ResNet 332-543), mmdet/models/shared_heads/res_layer.py (ResLayer 13-81), mmdet/models/backbones/resnext.py (the grouped
Bottleneck 12-91, ResNeXt 157-238) and mmdet/models/shared_heads/resx_layer.py (ResXLayer 15-57): same class names,
constructor kwargs, sub-module names and parameter shapes, so `build_from_cfg` and reference
checkpoints work unchanged.  The nn.Conv2d / nn.BatchNorm2d children only HOLD parameters; the
forward pass runs on packed device buffers:
  * activations are physical NHWC (exposed as logical NCHW `channels_last` tensors),
  * frozen BatchNorm (eval mode, eps 1e-5: mmdet/models/utils/norm.py:43) is folded into the
    conv weight / an f32 bias at pack time,
  * bias + residual add + ReLU run in the GEMM epilogue (one launch per conv, no BN/ReLU/add
    kernels; the reference issues ~4 launches per conv).
Inference only: BN layers are always treated as frozen (both configs set norm_eval=True,
requires_grad=False).  There is no CPU path (native.py raises on CPU tensors).
"""
import collections
import itertools
import math

import torch
import torch.nn as nn

from . import native
from .registry import BACKBONES, SHARED_HEADS

ARCH_SETTINGS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
STEM_KP = 192  # 7*7*3 = 147 patch elements padded to a K-step multiple


def as_nhwc(x, dtype):
    """Logical [B,C,H,W] tensor -> physical [B,H,W,C] contiguous tensor of `dtype` (no copy when it already is) at a 128-byte aligned
    address, which the routes planned by shape assume of a block input (16 bytes; split half 128): a view at any other address is copied."""
    v = x.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        return native.nchw_to_nhwc(x.contiguous(), dtype)
    v = v if x.dtype == dtype else native.cast(v, dtype)
    return v if v.data_ptr() % 128 == 0 else v.clone()


def as_logical(y):
    """Physical [B,H,W,C] -> logical [B,C,H,W] (channels_last strides, no copy)."""
    return y.permute(0, 3, 1, 2)


def fold_conv_bn(conv, bn, dtype):
    """(w [Cout,KH,KW,Cin] in `dtype`, bias [Cout] f32) with eval-mode BN folded in."""
    if bn is not None and conv.bias is None and dtype == torch.bfloat16 and conv.weight.is_cuda \
            and conv.weight.dtype == torch.float32 and conv.weight.is_contiguous() and not bn.training:
        # the same numbers in one launch (or none; bf16 only -- the half instance of the pack kernel rounds product and conversion in ONE
        # step, v_fma_mixlo_f16, where torch rounds twice: tools/probe_fold.py): the frozen BatchNorm's affine is cached until one of its tensors changes, and the
        # permute + scale + rounding is the pack kernel the training path uses -- inside a training iteration the operand this
        # iteration's weight table already holds (the no-grad res5 pass of HNMBRCNN.forward_train repacks after every update)
        from . import train_ops as TO
        s_, t_ = TO._frozen_bn_affine(bn)
        w_ = conv.weight.detach()
        eff = TO.table_operand(conv.weight, s_, tuple(w_.shape), dtype)
        return (eff if eff is not None else native.pack_conv_weight(w_, s_, dtype)), t_
    w = conv.weight.detach().float()
    if bn is not None:
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        bias = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
        w = w * scale[:, None, None, None]
    else:
        bias = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    if bn is not None and conv.bias is not None:
        bias = bias + conv.bias.detach().float() * scale
    return native.as_operand(w.permute(0, 2, 3, 1), dtype), bias.contiguous()


class PackedMixin(object):
    """Lazily packed device weights, rebuilt when the dtype/device changes or a state dict is loaded."""

    def _init_packed(self):
        self._packed = None
        self._packed_key = None
        self.compute_dtype = torch.bfloat16
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._drop_packed())

    def _drop_packed(self):
        if self._packed is not None:
            from . import graphs   # captured hipGraphs read the packed buffers by address: they must not replay after this
            graphs.invalidate_all('packed weights of %s were rebuilt' % type(self).__name__)
        self._packed = None
        self._packed_ready = None

    _packed_ready = None

    def packed(self, device):
        """The packed weights, built on first use.  The pack kernels run on the stream that first asks (with frame groups that
        is a SIDE stream: the host enqueues the side groups first); any other stream that uses the same tensors afterwards
        -- the main stream's group, a second window lane -- must be ordered behind them, or it reads weights that are still
        being written: an event recorded behind the pack, awaited once per consuming stream."""
        key = (self.compute_dtype, str(device))
        if self._packed is None or self._packed_key != key:
            with torch.no_grad():
                self._packed = self._pack(self.compute_dtype)
            self._packed_key = key
            self._packed_ready = None
            if getattr(device, 'type', None) == 'cuda':
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
                self._packed_ready = (ev, {native._raw_stream(device)})
        elif self._packed_ready is not None:
            ev, seen = self._packed_ready
            rs = native._raw_stream(device)
            if rs not in seen:
                torch.cuda.current_stream(device).wait_event(ev)
                seen.add(rs)
        return self._packed


def set_compute_dtype(module, dtype):
    """The operand format of every packed module below `module` -- the precision ladder of include/hvr_hip.h:
    torch.bfloat16 (benchmark dtype, every dedicated kernel), torch.float16 (half operands on the tile engine),
    native.SPLIT (split half: three half MFMAs per product, f32-grade results) or torch.float32 (exact-f32 MFMA).
    Modules convert their inputs on entry, so sub-trees may differ: e.g. set_compute_dtype(model.backbone, native.SPLIT)
    after set_compute_dtype(model, torch.float16)."""
    assert dtype in native.COMPUTE_DTYPES, dtype
    for m in module.modules():
        if isinstance(m, PackedMixin):
            m.compute_dtype = dtype
            m._drop_packed()
    return module


def enable_training(module):
    """Marks the parameters the reference trains as requires_grad (the builders freeze everything for inference):
    all conv / linear weights and biases EXCEPT BatchNorm parameters (norm_cfg requires_grad=False, norm_eval=True in both
    configs) and a ResNet's stem + first `frozen_stages` stages (resnet.py:484-494).  Use with
    set_compute_dtype(module, torch.float32); the forward_train_* methods then build autograd graphs of HIP ops."""
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            continue
        for p in m.parameters(recurse=False):
            p.requires_grad = True
    for m in module.modules():
        if isinstance(m, ResNet):
            frozen = [m.conv1, m.norm1] + [getattr(m, 'layer%d' % i) for i in range(1, m.frozen_stages + 1)]
            for f in frozen:
                for p in f.parameters():
                    p.requires_grad = False
    for m in module.modules():
        if type(m).__name__ == 'HNMBRCNN':
            # this detector's forward_train computes C4 under no_grad and never adds an RPN loss (hnmb_rcnn.py:269-283,318-325):
            # backbone and RPN parameters never receive a gradient there, and torch.optim.SGD skips gradient-less parameters
            # (no weight decay either) -- keep them out of the flat parameter set so the fused update leaves them alone too
            for part in (m.backbone, getattr(m, 'rpn_head', None)):
                if part is not None:
                    for p in part.parameters():
                        p.requires_grad = False
    return module


GN_GROUP_WIDTHS = (2, 4, 8, 16, 32, 64)   # channels per group the group-norm kernels take (include/hvr_hip.h: hvr_gn_supported)


def norm_kind(norm_cfg, what):
    """norm_cfg -> ('BN', None, eps) or ('GN', num_groups, eps), as build_norm_layer reads it (norm.py:12-55); every other type is refused."""
    cfg = norm_cfg if norm_cfg is not None else dict(type='BN')
    kind = cfg.get('type', 'BN')
    if kind == 'BN':
        return 'BN', None, cfg.get('eps', 1e-5)
    if kind != 'GN':
        raise NotImplementedError('%s: norm_cfg type %r is not built (frozen BatchNorm \'BN\' and GroupNorm \'GN\' are)' % (what, kind))
    assert 'num_groups' in cfg, '%s: norm_cfg type GN needs num_groups' % what
    return 'GN', int(cfg['num_groups']), cfg.get('eps', 1e-5)


def gn_padded(C, G, what):
    """(channels, groups) of the map the group-norm kernels run for a GroupNorm(G, C): C rounded up to a multiple of 64 with whole groups of
    exact zeros behind the real ones (weight rows, gamma and beta 0: such a group normalises to exact zeros), or NotImplementedError where
    the instance set of include/hvr_hip.h has no such form."""
    if G < 1 or C % G or C // G not in GN_GROUP_WIDTHS or C > 2048:
        raise NotImplementedError('%s: GroupNorm with num_groups=%d on %d channels is outside the kernels\' instance set (num_groups divides the '
                                  'channels, channels per group in %s, up to 2048 channels)' % (what, G, C, list(GN_GROUP_WIDTHS)))
    Cp = (C + 63) // 64 * 64
    return Cp, Cp // (C // G)


def _pad_to(t, shape):
    """t in the leading corner of a zero tensor of `shape`."""
    if tuple(t.shape) == tuple(shape):
        return t.contiguous()
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


class Step(collections.namedtuple('Step', 'kind projection downsample stride compact h1_in', defaults=(False, False, None, False, False))):
    """How one Bottleneck of a stage closes (ResNet.stage_route).  kind: the native entry -- 'tail', 'tail_next' (`projection`: the shortcut
    as a second K segment, else the identity form), 'tail_next_live', 'close_sampled' (at `stride` 2 from the full-resolution input), 'conv',
    'gcb' (a block with a context block: the closing 1x1 without residual or ReLU, then native.context_block with both) or 'gn' (a block
    under GroupNorm: every conv raw, its norm two launches behind it, the residual add and the ReLU in the last norm's apply).
    downsample: the projection shortcut is a conv of its own in front.  compact ('close_sampled' at stride 1, 'conv'): the dense close on the
    compact map that a tail_next_live block left.  h1_in: the block's conv1 output arrived from the block before."""

    def __str__(self):
        form = {'tail_next': '(projection)' if self.projection else '(identity)', 'close_sampled': '/%s' % self.stride}.get(self.kind, '')
        return ('downsample+' if self.downsample else '') + self.kind + form + ('@compact' if self.compact and self.kind == 'conv' else '')


class Route(collections.namedtuple('Route', 'steps out_hw compact')):
    """A stage's Steps (one per block), the (H, W) of the map it stores, and whether that is the compact map: the stage output at [:, ::2, ::2]."""

    def __str__(self):
        runs = [(k, len(list(g))) for k, g in itertools.groupby(str(s) for s in self.steps)]
        return '%s -> %dx%d%s' % (', '.join(k if n == 1 else '%s x%d' % (k, n) for k, n in runs), self.out_hw[0], self.out_hw[1],
                                  ' compact' if self.compact else '')


def _w2d(wb):
    """A packed 1x1 conv (w [Cout,1,1,Cin], bias) as the fused entries take it: (w [Cout,Cin], bias)."""
    return wb[0].reshape(wb[0].shape[0], -1), wb[1]


class Bottleneck(nn.Module, PackedMixin):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', norm_cfg=None, dcn=None, groups=1, base_width=4,
                 gcb=None, gen_attention=None):
        super(Bottleneck, self).__init__()
        assert style in ['pytorch', 'caffe']
        assert dcn is None or isinstance(dcn, dict)
        assert gcb is None or isinstance(gcb, dict)
        assert gen_attention is None or isinstance(gen_attention, dict)
        self.inplanes, self.planes, self.stride, self.dilation, self.style = inplanes, planes, stride, dilation, style
        # resnext.py:21-24: the channels of conv1's output, conv2 and conv3's input (a ResNet block: planes)
        self.groups, self.base_width = groups, base_width
        self.width = width = planes if groups == 1 else int(math.floor(planes * (base_width / 64))) * groups
        if groups > 1 and dcn is not None:
            raise NotImplementedError('dcn on a grouped Bottleneck (the dcn[\'groups\'] form of resnext.py:57-83) is not built')
        if groups > 1 and gen_attention is not None:
            raise NotImplementedError('gen_attention on a grouped Bottleneck is not built (the reference\'s resnext.py accepts the argument and drops it)')
        kind, self.num_groups, eps = norm_kind(norm_cfg, 'Bottleneck')
        self.with_gn = kind == 'GN'
        if self.with_gn:
            for arg, name in ((dcn, 'dcn'), (gcb, 'gcb'), (gen_attention, 'gen_attention')):
                if arg is not None:
                    raise NotImplementedError('%s on a Bottleneck under GroupNorm (norm_cfg type GN) is not built' % name)
            if groups > 1:
                raise NotImplementedError('GroupNorm (norm_cfg type GN) on a grouped Bottleneck (groups=%d) is not built' % groups)
            # the maps the norms run on: conv1 / conv2 outputs (width channels, padded with zero groups to a multiple of 64) and conv3's
            self.gn_width, self.gn_width_groups = gn_padded(width, self.num_groups, 'Bottleneck gn1 / gn2')
            if gn_padded(planes * 4, self.num_groups, 'Bottleneck gn3') != (planes * 4, self.num_groups):
                raise NotImplementedError('Bottleneck gn3: %d channels are no multiple of 64 (GroupNorm kernels)' % (planes * 4))
            if downsample is not None and not isinstance(downsample[1], nn.GroupNorm):
                raise NotImplementedError('a Bottleneck under GroupNorm takes a (conv, GroupNorm) projection shortcut, got %s' % type(downsample[1]).__name__)
        self.gn_eps = eps
        self.norm_names = tuple(('gn' if self.with_gn else 'bn') + str(i) for i in (1, 2, 3))

        def norm(ch):   # norm.py: build_norm_layer
            return nn.GroupNorm(self.num_groups, ch, eps=eps) if self.with_gn else nn.BatchNorm2d(ch, eps=eps)
        # caffe: stride on the first 1x1 (resnet.py:127-132)
        self.conv1_stride, self.conv2_stride = (1, stride) if style == 'pytorch' else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, width, 1, stride=self.conv1_stride, bias=False)
        self.add_module(self.norm_names[0], norm(width))
        # resnet.py:147-186: conv2 is a (modulated) deformable 3x3 whose offsets (and mask logits) come from conv2_offset, a plain
        # biased 3x3 on the same input; fallback_on_stride keeps the plain conv where conv2 carries a stride
        self.dcn = dcn
        self.with_dcn = dcn is not None and not (dcn.get('fallback_on_stride', False) and self.conv2_stride > 1)
        self.with_modulated_dcn = self.with_dcn and bool(dcn.get('modulated', False))
        self.deformable_groups = int(dcn.get('deformable_groups', 1)) if self.with_dcn else 1
        if self.with_dcn:
            offset_channels = 27 if self.with_modulated_dcn else 18
            self.conv2_offset = nn.Conv2d(width, self.deformable_groups * offset_channels, 3, stride=self.conv2_stride, padding=dilation,
                                          dilation=dilation)
        self.conv2 = nn.Conv2d(width, width, 3, stride=self.conv2_stride, padding=dilation, dilation=dilation, groups=groups, bias=False)
        self.add_module(self.norm_names[1], norm(width))
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.add_module(self.norm_names[2], norm(planes * 4))
        self.downsample = downsample
        # resnet.py:199-201,249-250: the global context block acts on bn3's output, in front of the residual add
        self.gcb, self.with_gcb = gcb, gcb is not None
        if self.with_gcb:
            from .ops import ContextBlock   # (ops imports this module)
            self.context_block = ContextBlock(inplanes=planes * self.expansion, **gcb)
        # resnet.py:203-206,243-244: the generalized attention block acts on relu(bn2(conv2)), in front of conv3
        self.gen_attention, self.with_gen_attention = gen_attention, gen_attention is not None
        if self.with_gen_attention:
            from .ops import GeneralizedAttention   # (ops imports this module)
            self.gen_attention_block = GeneralizedAttention(planes, **gen_attention)
        self._init_packed()

    norm1 = property(lambda self: getattr(self, self.norm_names[0]))   # resnet.py:208-218
    norm2 = property(lambda self: getattr(self, self.norm_names[1]))
    norm3 = property(lambda self: getattr(self, self.norm_names[2]))

    def _pack_gn(self, dtype):
        """Under GroupNorm nothing folds: the conv weights raw (no bias), gamma and beta f32.  Where width is no multiple of 64 the maps of
        conv1 and conv2 carry whole groups of zero channels behind the real ones (gn_padded): zero weight rows and columns, gamma = beta = 0."""
        wp = self.gn_width

        def raw(conv, cout, cin):
            w = conv.weight.detach().float().permute(0, 2, 3, 1)
            return native.as_operand(_pad_to(w, (cout, w.shape[1], w.shape[2], cin)), dtype)

        def affine(gn, c):
            return _pad_to(gn.weight.detach().float(), (c,)), _pad_to(gn.bias.detach().float(), (c,))
        p = dict(c1=raw(self.conv1, wp, self.inplanes), n1=affine(self.norm1, wp), c2=raw(self.conv2, wp, wp), n2=affine(self.norm2, wp),
                 c3=raw(self.conv3, 4 * self.planes, wp), n3=affine(self.norm3, 4 * self.planes))
        if self.downsample is not None:
            p['ds'], p['nd'] = raw(self.downsample[0], 4 * self.planes, self.inplanes), affine(self.downsample[1], 4 * self.planes)
        return p

    def _pack(self, dtype):
        if self.with_gn:
            return self._pack_gn(dtype)
        p = dict(c1=fold_conv_bn(self.conv1, self.norm1, dtype), c3=fold_conv_bn(self.conv3, self.norm3, dtype))
        if self.groups > 1:
            # bn2 folded into the grouped weight [width,3,3,width/groups]; the operand forms (grouped, block-diagonal dense) are made by the
            # route that first needs them (native.GroupedWeight)
            wg, bg = fold_conv_bn(self.conv2, self.norm2, torch.float32)
            p['c2'] = (native.GroupedWeight(wg, dtype), bg)
        else:
            p['c2'] = fold_conv_bn(self.conv2, self.norm2, dtype)
        if self.with_dcn:
            # the offset conv: Cout padded with zero rows to a multiple the engine takes (N % 4); its output stays f32 in every mode
            wo, bo = fold_conv_bn(self.conv2_offset, None, torch.float32)
            n = wo.shape[0]
            npad = (n + 3) // 4 * 4
            wp = torch.zeros((npad,) + tuple(wo.shape[1:]), dtype=torch.float32, device=wo.device)
            bp = torch.zeros((npad,), dtype=torch.float32, device=wo.device)
            wp[:n], bp[:n] = wo, bo
            p['off'] = (native.as_operand(wp, dtype), bp)
        if self.downsample is not None:
            p['ds'] = fold_conv_bn(self.downsample[0], self.downsample[1], dtype)
            # the projection shortcut as a second K segment of the closing 1x1 (hvr_bottleneck_tail): rows [W3 | Wd]
            p['tail'] = (torch.cat([p['c3'][0].reshape(p['c3'][0].shape[0], -1), p['ds'][0].reshape(p['ds'][0].shape[0], -1)], 1).contiguous(),
                         (p['c3'][1] + p['ds'][1]).contiguous())
        return p

    # ---- the steps of a block.  Which close runs is planned by shape (plan_close, ResNet.stage_route); a step runs its entry or raises.
    def plan_close(self, B, H, W, dtype, nxt=None, compact_in=False):
        """The Step this block closes through at full resolution on a [B,H,W] input map (pure: shape queries, nothing launched); the conv1 of
        nxt, the block that reads the output, rides on the close where hvr_bottleneck_tail_next has a kernel."""
        stride = 1 if compact_in else self.stride
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        P, C, proj = self.width, 4 * self.planes, self.downsample is not None
        if self.with_gn:    # a group's statistics need every pixel of the conv's output: no fused close, no sampled or compact form
            return Step('gn', downsample=proj)
        if self.with_gcb:   # the context block sits between conv3 and the residual add: no fused close, whatever fuse_next / fuse_tail say
            return Step('gcb', downsample=proj)
        # split half has no second-K-segment tail: the projection is its own conv and enters the fused closing 1x1 + next conv1 as the
        # residual (the identity form of hvr_bottleneck_tail_next)
        own_ds = proj and dtype == native.SPLIT
        x_hwc = (H, W, self.inplanes) if proj and not own_ds else None
        if nxt is not None and self.fuse_next and nxt.conv1_stride == 1 and (own_ds or self.fuse_tail or not proj) \
                and native.tail_next_path(B, OH, OW, P, C, nxt.width, x_hwc, stride, dtype):
            return Step('tail_next', projection=x_hwc is not None, downsample=own_ds)
        if x_hwc is not None and self.fuse_tail and native.tail_path(B, OH, OW, P, C, x_hwc, stride, dtype):
            return Step('tail')
        return Step('conv', downsample=proj)

    def body(self, x, h1=None, compact_in=False, conv2_stride=None, out=None, conv2_only=False):
        """conv1 (unless h1, its output, was handed in by the block before) and conv2 or the deformable pair -> the closing 1x1's input.
        compact_in (a caffe-style stride-2 block): x holds only the pixels the strided 1x1 convs read, so they run at stride 1.
        A block with a generalized attention block applies it here, to conv2's output at every pixel (conv2_only: without it): every close
        that only reads h ('conv', 'tail', 'tail_next', 'gcb') stays available to it; the sampled and compact forms are not (ResNet._dead_pixels)."""
        if self.with_gn:
            assert h1 is None and not compact_in and conv2_stride is None and out is None, 'a block under GroupNorm has the full-resolution form only'
            p = self.packed(x.device)
            h = self._gn(self._gn_conv(x, p['c1'], stride=self.conv1_stride), p['n1'], self.gn_width_groups, x.dtype)
            u = self._gn_conv(h, p['c2'], stride=self.conv2_stride, pad=self.dilation, dil=self.dilation)
            return self._gn(u, p['n2'], self.gn_width_groups, x.dtype)
        if self.with_gen_attention and not conv2_only:
            assert conv2_stride is None, 'a block with gen_attention has no sampled form'
            return self.gen_attention_block.forward_nhwc(self.body(x, h1, compact_in, conv2_only=True), out=out)
        p = self.packed(x.device if h1 is None else h1.device)
        h = h1 if h1 is not None else native.conv2d_nhwc(x, p['c1'][0], p['c1'][1], relu=True, stride=1 if compact_in else self.conv1_stride)
        s2 = self.conv2_stride if conv2_stride is None else conv2_stride
        if self.with_dcn:
            om = native.conv2d_nhwc(h, p['off'][0], p['off'][1], relu=False, stride=s2, pad=self.dilation, dil=self.dilation, out_f32=True)
            return native.deform_conv2d_nhwc(h, om, p['c2'][0], p['c2'][1], True, s2, self.dilation, self.dilation, self.deformable_groups,
                                             self.with_modulated_dcn, out=out)
        if self.groups > 1:
            return native.conv3x3_grouped(h, p['c2'][0], p['c2'][1], True, s2, self.dilation, out=out, route=self.grouped_route)
        return native.conv2d_nhwc(h, p['c2'][0], p['c2'][1], relu=True, stride=s2, pad=self.dilation, dil=self.dilation, out=out)

    @staticmethod
    def _gn_conv(x, w, **kw):
        """A raw conv (no bias, no activation) -> u in the format its norm reads: the compute format (one rounding of u more than the
        reference makes, as the context block's u), split half: f32 straight from the accumulators."""
        return native.conv2d_nhwc(x, w, None, relu=False, out_f32=x.dtype == native.SPLIT, **kw)

    def _gn(self, u, affine, G, dtype, relu=True, resid=None, resid_norm=None, out=None):
        """GroupNorm (+ r) (+ ReLU) on u -> a map in the compute format `dtype`: in place on u, or into out.  Split half has no kernel form: u
        is f32, the result is cast (the rule the context block follows)."""
        if dtype == native.SPLIT:
            y = native.cast(native.group_norm(u, affine[0], affine[1], G, self.gn_eps, resid, resid_norm, relu, out=u), native.SPLIT)
            if out is None:
                return y
            out.copy_(y)
            return out
        return native.group_norm(u, affine[0], affine[1], G, self.gn_eps, resid, resid_norm, relu, out=u if out is None else out)

    def _conv2(self, x, h1, compact_in, conv2_stride, out):
        return self.body(x, h1, compact_in, conv2_stride, out, conv2_only=True)

    def close(self, x, h, step, out=None, compact_in=False):
        """The plain close ('tail', 'conv' or 'gcb') -> y.  out: where y goes (a contiguous [B,OH,OW,4*planes] tensor), e.g. a frame group's slice."""
        p = self.packed(x.device)
        stride = 1 if compact_in else self.stride
        if step.kind == 'gn':
            # y = relu(GN3(conv3(h)) + identity) in ONE apply; a projection shortcut's conv output is normalised inside it (its statistics
            # are one more pass, its normalised map is never written)
            assert self.with_gn and not compact_in, step
            G, u = self.num_groups, self._gn_conv(h, p['c3'])
            if step.downsample:
                resid = self._gn_conv(x, p['ds'], stride=stride)
                rn = (native.group_norm_stats(resid, G),) + p['nd']
            else:
                resid, rn = native.cast(x, torch.float32) if x.dtype == native.SPLIT else x, None
            return self._gn(u, p['n3'], G, x.dtype, True, resid, rn, out)
        if step.kind == 'gcb':
            # u = bn3(conv3(h)) as a map of its own (the pool reads every pixel of it), then relu(context_block(u) + identity) in the apply
            identity = native.conv2d_nhwc(x, p['ds'][0], p['ds'][1], relu=False, stride=stride) if step.downsample else x
            u = native.conv2d_nhwc(h, p['c3'][0], p['c3'][1], relu=False)
            return self.context_block.forward_nhwc(u, resid=identity, relu=True, out=out)
        if step.kind == 'tail':
            # relu(conv3(h) + downsample(x)) in one pass: the identity map is never written (resnet.py:248-264)
            return native.bottleneck_tail(h, x, p['tail'][0], p['tail'][1], stride2=stride, relu=True, out=out)
        assert step.kind == 'conv' and not step.compact, step
        identity = native.conv2d_nhwc(x, p['ds'][0], p['ds'][1], relu=False, stride=stride) if step.downsample else x
        return native.conv2d_nhwc(h, p['c3'][0], p['c3'][1], resid=identity, relu=True, out=out)

    def close_next(self, x, h, nxt, step, compact_in=False):
        """'tail_next' -> (y, nxt's conv1 output)."""
        p, (wn, bn) = self.packed(x.device), _w2d(nxt.packed(x.device)['c1'])
        stride = 1 if compact_in else self.stride
        if step.projection:
            return native.bottleneck_tail_next(h, x, None, p['tail'][0], p['tail'][1], wn, bn, stride2=stride)
        identity = native.conv2d_nhwc(x, p['ds'][0], p['ds'][1], relu=False, stride=stride) if step.downsample else x
        return native.bottleneck_tail_next(h, None, identity, *_w2d(p['c3']), wn, bn, stride2=1)

    def close_next_live(self, x, h, nxt, live_stride=2):
        """'tail_next_live': an identity block whose output nothing reads but nxt's conv1 and a stride-s consumer (s = live_stride)
        -> (y_live [B,(H-1)//s+1,(W-1)//s+1,4*planes] = the output at [:, ::s, ::s], nxt's conv1 output at full resolution)."""
        (w3, b3), (wn, bn) = _w2d(self.packed(x.device)['c3']), _w2d(nxt.packed(x.device)['c1'])
        return native.bottleneck_tail_next_live(h, x, w3, b3, wn, bn, live_stride=live_stride)

    def close_sampled(self, x, h1=None, stride=2):
        """'close_sampled' at stride 2, the whole of an identity block whose output only a stride-`stride` 1x1 consumer reads: conv1 everywhere (the
        3x3 reads neighbours), conv2 at that stride, the close with the residual sampled from x -> the full output at [:, ::stride, ::stride]."""
        assert self.downsample is None and self.stride == 1 and not self.with_dcn and not self.with_gen_attention
        B, H, W, _ = x.shape
        hs = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, self.width), dtype=x.dtype, device=x.device)
        self.body(x, h1, conv2_stride=stride, out=hs)
        return native.bottleneck_close_sampled(hs, *_w2d(self.packed(x.device)['c3']), x, stride=stride, relu=True)

    def close_compact(self, x_live, h1, stride=2, plain=False):
        """The same block behind close_next_live: x_live is its input at [:, ::stride, ::stride] only, h1 its conv1 output at full resolution,
        and the close is dense on the compact map: 'close_sampled' at stride 1, or with `plain` 'conv' (the same row-panel kernel and sums)."""
        assert self.downsample is None and self.stride == 1 and not self.with_dcn and not self.with_gen_attention
        assert tuple(x_live.shape[1:3]) == ((h1.shape[1] - 1) // stride + 1, (h1.shape[2] - 1) // stride + 1)
        w3, b3 = self.packed(h1.device)['c3']
        hs = self.body(None, h1, conv2_stride=stride)
        if plain:
            return native.conv2d_nhwc(hs, w3, b3, resid=x_live, relu=True)
        return native.bottleneck_close_sampled(hs, w3.reshape(w3.shape[0], -1), b3, x_live, stride=1, relu=True)

    def forward_nhwc(self, x, out=None, h1=None):
        """The block on its own, at full resolution: body + plain close -> y.  out as in close, h1 as in body."""
        return self.close(x, self.body(x, h1), self.plan_close(x.shape[0], x.shape[1], x.shape[2], x.dtype), out=out)

    fuse_next = True   # class attributes (tests flip them to compare the fused kernels with the per-conv path); no environment switch
    fuse_tail = True
    grouped_route = None   # conv2 of a grouped block: None = native.conv3x3_grouped chooses by shape; 'grouped' / 'dense' force one (tests, tools)

    def forward(self, x):
        return as_logical(self.forward_nhwc(as_nhwc(x, self.compute_dtype)))

    def forward_train_nhwc(self, x):
        """The block as an autograd graph of HIP convs (train_ops.conv_bn): frozen BatchNorm statistics and affine
        (norm_eval=True, requires_grad=False in both configs), trainable conv weights; f32, physical NHWC."""
        if self.with_gn:
            raise NotImplementedError('Bottlenecks under GroupNorm are inference only: group normalisation has no backward')
        if self.with_dcn:
            raise NotImplementedError('deformable convs are inference only: no backward (col2im + coordinate gradients) is implemented')
        if self.groups > 1:
            raise NotImplementedError('grouped Bottlenecks are inference only: the grouped 3x3 conv has no backward')
        if self.with_gcb:
            raise NotImplementedError('Bottlenecks with a context block are inference only: the pool has no backward')
        if self.with_gen_attention:
            raise NotImplementedError('Bottlenecks with a generalized attention block are inference only: the attention core has no backward')
        from . import train_ops as TO
        out = TO.conv_bn(x, self.conv1, self.norm1, relu=True)
        out = TO.conv_bn(out, self.conv2, self.norm2, relu=True)
        identity = x if self.downsample is None else TO.conv_bn(x, self.downsample[0], self.downsample[1])
        return TO.conv_bn(out, self.conv3, self.norm3, resid=identity, relu=True)


def make_res_layer(block, inplanes, planes, blocks, stride=1, dilation=1, style='pytorch', norm_cfg=None, dcn=None, groups=1, base_width=4, gcb=None,
                   gen_attention=None, gen_attention_blocks=(), **_unused):
    downsample = None
    kind, num_groups, eps = norm_kind(norm_cfg, 'make_res_layer')
    if stride != 1 or inplanes != planes * block.expansion:
        cout = planes * block.expansion
        downsample = nn.Sequential(nn.Conv2d(inplanes, cout, 1, stride=stride, bias=False),
                                   nn.GroupNorm(num_groups, cout, eps=eps) if kind == 'GN' else nn.BatchNorm2d(cout, eps=eps))
    extra = {} if dcn is None else dict(dcn=dcn)
    if groups != 1:   # resnext.py:94-154
        extra.update(groups=groups, base_width=base_width)
    if gcb is not None:
        extra.update(gcb=gcb)

    def att(i):   # resnet.py:310-327: the blocks of the stage named in gen_attention_blocks
        return dict(gen_attention=gen_attention) if gen_attention is not None and i in gen_attention_blocks else {}
    layers = [block(inplanes, planes, stride, dilation, downsample, style=style, norm_cfg=norm_cfg, **extra, **att(0))]
    inplanes = planes * block.expansion
    for i in range(1, blocks):
        layers.append(block(inplanes, planes, 1, dilation, style=style, norm_cfg=norm_cfg, **extra, **att(i)))
    return nn.Sequential(*layers)


def _freeze(module):
    module.eval()
    for p in module.parameters():
        p.requires_grad = False


@BACKBONES.register_module
class ResNet(nn.Module, PackedMixin):
    """Same kwargs as the reference ResNet (resnet.py:372-395); dcn / stage_with_dcn as there (deformable conv2 in the marked
    stages, inference only); gcb / stage_with_gcb as there (a global context block between bn3 and the residual add of every block of the
    marked stages, inference only); gen_attention / stage_with_gen_attention as there (a generalized attention block between conv2 and conv3
    of the blocks named per stage, inference only); norm_cfg type 'BN' (frozen, folded into the convs) or 'GN' (dict(type='GN',
    num_groups=32): gn1 / gn2 / gn3 as in the reference, native.group_norm behind every raw conv, inference only, not together with dcn /
    gcb / gen_attention); conv_cfg must be None."""
    arch_settings = {d: (Bottleneck, s) for d, s in ARCH_SETTINGS.items()}
    _block_kwargs = {}   # what every block gets beyond the reference ResNet's arguments (ResNeXt: groups, base_width)

    def __init__(self, depth, in_channels=3, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), gcb=None, stage_with_gcb=(False, False, False, False),
                 gen_attention=None, stage_with_gen_attention=((), (), (), ()), with_cp=False, zero_init_residual=True):
        super(ResNet, self).__init__()
        if depth not in self.arch_settings:
            raise KeyError('invalid depth {} for resnet'.format(depth))
        if conv_cfg is not None:
            raise NotImplementedError('conv_cfg is outside the HVR hot path')
        block, stage_blocks = self.arch_settings[depth]
        if gen_attention is not None:
            assert isinstance(gen_attention, dict), gen_attention
            marked = [tuple(stage_with_gen_attention[i]) if i < len(stage_with_gen_attention) else () for i in range(num_stages)]
            for i, idx in enumerate(marked):
                for j in idx:
                    if not 0 <= j < stage_blocks[i]:
                        raise ValueError('stage_with_gen_attention[%d] names block %r, stage %d of depth %d has blocks 0 .. %d: the reference would '
                                         'build no attention block there and say nothing' % (i, j, i + 1, depth, stage_blocks[i] - 1))
            if not any(marked):
                # (the reference builds the plain net then and drops the dict without a word; an argument that would be disobeyed is refused)
                raise NotImplementedError('gen_attention is given but stage_with_gen_attention marks no block: no attention block would be built; '
                                          'mark a block or pass gen_attention=None')
        self.gen_attention, self.stage_with_gen_attention = gen_attention, stage_with_gen_attention
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
        self.dcn, self.stage_with_dcn = dcn, stage_with_dcn
        if gcb is not None:
            assert len(stage_with_gcb) == num_stages
            if not any(stage_with_gcb):
                # (the reference builds the plain net then and drops the dict without a word; an argument that would be disobeyed is refused)
                raise NotImplementedError('gcb is given but stage_with_gcb marks no stage: no context block would be built; mark a stage or pass gcb=None')
        self.gcb, self.stage_with_gcb = gcb, stage_with_gcb
        kind, self.num_groups, eps = norm_kind(norm_cfg, type(self).__name__)
        self.with_gn, self.gn_eps, self.norm_cfg = kind == 'GN', eps, norm_cfg
        if self.with_gn:
            for arg, name in ((dcn, 'dcn'), (gcb, 'gcb'), (gen_attention, 'gen_attention')):
                if arg is not None:
                    raise NotImplementedError('%s together with GroupNorm (norm_cfg type GN) is not built' % name)
            if self._block_kwargs.get('groups', 1) > 1:
                raise NotImplementedError('GroupNorm (norm_cfg type GN) on %s with groups=%d is not built' % (type(self).__name__, self._block_kwargs['groups']))
            if gn_padded(64, self.num_groups, 'the stem\'s gn1') != (64, self.num_groups):
                raise NotImplementedError('the stem\'s gn1: num_groups=%d on 64 channels is outside the instance set' % self.num_groups)
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        assert in_channels == 3
        self.depth, self.num_stages, self.strides, self.dilations = depth, num_stages, strides, dilations
        self.out_indices, self.style, self.frozen_stages, self.norm_eval = out_indices, style, frozen_stages, norm_eval
        self.zero_init_residual = zero_init_residual
        self.stage_blocks = stage_blocks[:num_stages]
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.norm1_name = 'gn1' if self.with_gn else 'bn1'
        self.add_module(self.norm1_name, nn.GroupNorm(self.num_groups, 64, eps=eps) if self.with_gn else nn.BatchNorm2d(64, eps=eps))
        self.res_layers = []
        inplanes = 64
        for i, nb in enumerate(self.stage_blocks):
            planes = 64 * 2 ** i
            name = 'layer{}'.format(i + 1)
            stage_dcn = dcn if dcn is not None and stage_with_dcn[i] else None
            stage_gcb = gcb if gcb is not None and stage_with_gcb[i] else None
            stage_att = tuple(stage_with_gen_attention[i]) if gen_attention is not None and i < len(stage_with_gen_attention) else ()
            self.add_module(name, make_res_layer(block, inplanes, planes, nb, stride=strides[i], dilation=dilations[i],
                                                 style=style, norm_cfg=norm_cfg, dcn=stage_dcn, gcb=stage_gcb,
                                                 **(dict(gen_attention=gen_attention, gen_attention_blocks=stage_att) if stage_att else {}),
                                                 **self._block_kwargs))
            inplanes = planes * block.expansion
            self.res_layers.append(name)
        self.feat_dim = block.expansion * 64 * 2 ** (len(self.stage_blocks) - 1)
        self.fused_stem = True  # bf16 only: conv1 + bn1 + relu + maxpool in one kernel
        _freeze(self)
        self._init_packed()

    norm1 = property(lambda self: getattr(self, self.norm1_name))   # resnet.py:465-467

    def init_weights(self, pretrained=None):
        """resnet.py:496-520 (pretrained checkpoints are loaded by the caller via load_state_dict)."""
        if pretrained is not None:
            raise NotImplementedError('load checkpoints with load_state_dict (keys match the reference)')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.dcn is not None:   # resnet.py:507-511: a deformable conv starts as the plain conv (zero offsets; modulated: mask 0.5)
            for m in self.modules():
                if isinstance(m, Bottleneck) and m.with_dcn:
                    nn.init.constant_(m.conv2_offset.weight, 0)
                    nn.init.constant_(m.conv2_offset.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.norm3.weight, 0)
        set_compute_dtype(self, self.compute_dtype)

    def _pack(self, dtype):
        w, b = fold_conv_bn(self.conv1, None if self.with_gn else self.norm1, torch.float32)  # [64,7,7,3]
        wp = torch.zeros((64, STEM_KP), dtype=torch.float32, device=w.device)
        wp[:, :147] = w.reshape(64, 147)
        if self.with_gn:   # the raw weight for the patch-matrix GEMM (the fused stem kernel folds a BatchNorm: not used), gamma and beta f32
            return dict(stem=(native.as_operand(wp, dtype), None),
                        gn=(self.norm1.weight.detach().float().contiguous(), self.norm1.bias.detach().float().contiguous()))
        # fused bf16 stem: [n][ky][kx*4 + c], zero weight for the pad channel (c = 3) and the pad tap (kx = 7)
        wf = torch.zeros((64, 7, 8, 4), dtype=torch.float32, device=w.device)
        wf[:, :, :7, :3] = w
        if dtype == native.SPLIT:
            fused, fused_bias = native.stem_split_weights(wf.view(64, 7, 32)), native.stem_split_bias(b)
        else:
            fused, fused_bias = wf.view(64, 7, 32).to(dtype if dtype in (torch.bfloat16, torch.float16) else torch.bfloat16).contiguous(), b
        return dict(stem=(native.as_operand(wp, dtype), b), fused=fused, fused_bias=fused_bias)

    def out_shape_nhwc(self, B, H, W):
        """Physical [B,h,w,C] shape of the LAST returned map for a [B,3,H,W] input (stem 7x7/2 + pool 3x3/2, then one
        stride per stage), or None when the net returns several maps."""
        if len(self.out_indices) != 1:
            return None
        last = self.out_indices[0]
        h, w = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        for i in range(last + 1):
            h, w = (h - 1) // self.strides[i] + 1, (w - 1) // self.strides[i] + 1
        return (B, h, w, 64 * 2 ** last * 4)

    skip_dead_pixels = True   # class attribute (tests flip it to compare with the full-resolution path); no environment switch
    # Stages that end compact through 'close_sampled' (stage_route).  Layer 2 (index 1) qualifies too and is bit-identical as well
    # (tests/test_dead_pixels_gpu.py), but is not listed: in a bf16 window its 'conv' close on the compact map is the only closing conv that
    # hvr_conv2d_nhwc runs on the row-panel kernel, the route the forward-kernel census (tests/test_forward_kernels_gpu.py) checks against
    # f64, and as 'close_sampled' it would leave that entry (asserted on the route table: tests/test_stage_routes.py)
    compact_stages = (0,)
    # Stages whose block before the last writes only the live quarter of its output ('tail_next_live'), so that the last block closes
    # densely on the compact map: through 'close_sampled' at stride 1 where the stage is in compact_stages too, else -- layer 2 -- through 'conv'
    live_store_stages = (0, 1)

    def stage_route(self, i, B, H, W, dtype, compact_in=False):
        """The Route of stage i on a stored [B,H,W] input map (compact_in: the compact map the stage before left).  Pure: module structure, the
        class-attribute knobs, native.fewrow_enabled() and shape queries in; no tensors, nothing launched, nothing cached (str(route) prints it).
        Precedence: the live-store form and the dense close behind it, else the sampled close, else full resolution."""
        blocks = list(getattr(self, self.res_layers[i]))
        steps = []
        for j, blk in enumerate(blocks):
            nxt = blocks[j + 1] if j + 1 < len(blocks) else None
            first = compact_in and j == 0
            if j >= 1 and j + 2 == len(blocks) and self._live_store(i, blk, nxt, B, H, W, dtype):
                step = Step('tail_next_live')
            elif steps and steps[-1].kind == 'tail_next_live':
                step = Step('close_sampled', stride=1, compact=True) if i in self.compact_stages else Step('conv', compact=True)
            elif nxt is None and self._ends_compact(i) and dtype in native.FUSED_DTYPES \
                    and native.conv2d_path(B, H, W, blk.width, 4 * blk.planes, dtype=dtype, tile=native.TILE_HINT) == 1 \
                    and native.close_sampled_path(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, blk.width, 4 * blk.planes, H, W, 2, dtype):
                # (the sampled close is the row-panel kernel: the same sums as the full-resolution close only where that one takes it too)
                step = Step('close_sampled', stride=2)
            else:
                step = blk.plan_close(B, H, W, dtype, nxt, first)
            steps.append(step._replace(h1_in=bool(steps) and steps[-1].kind in ('tail_next', 'tail_next_live')))
            if not first:
                H, W = (H - 1) // blk.stride + 1, (W - 1) // blk.stride + 1
        compact = steps[-1].kind == 'close_sampled' or steps[-1].compact
        return Route(tuple(steps), ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if compact else (H, W), compact)

    def _ends_compact(self, i):
        return i in self.compact_stages and self._dead_pixels(i)

    def _live_store(self, i, blk, last, B, H, W, dtype):
        """True when stage i ends compact through the live-store form on a [B,H,W] map: blk, the block before the last, is an identity block
        whose output only `last` reads (conv1 from registers, the residual at the live pixels), both kernels exist, the compact map has the
        128 pixels of one panel, and the row-panel kernel takes the close at both sizes (its K order does not depend on the row count)."""
        if i not in self.live_store_stages or not self._dead_pixels(i) or not blk.fuse_next or dtype not in native.FUSED_DTYPES \
                or blk.downsample is not None or blk.stride != 1 or blk.with_dcn or blk.groups > 1 or last.conv1_stride != 1 \
                or blk.with_gcb or last.with_gcb:
            return False   # (a context block pools over every pixel of its block's map: nothing of a gcb stage is compacted)
        P, C, LH, LW = blk.width, 4 * blk.planes, (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if not native.tail_next_live_path(B, H, W, P, C, last.width, 2, dtype) or B * LH * LW < 128 \
                or native.conv2d_path(B, H, W, P, C, dtype=dtype, tile=native.TILE_HINT) != 1:
            return False
        if i in self.compact_stages:
            return native.close_sampled_path(B, LH, LW, P, C, LH, LW, 1, dtype)
        return native.conv2d_path(B, LH, LW, P, C, dtype=dtype, tile=native.TILE_HINT) == 1

    def _dead_pixels(self, i):
        """True when nothing reads stage i's output but the stride-2 1x1 convs (conv1 and downsample) of a caffe-style stage i + 1
        (resnet.py:127-132,283-296): three quarters of its pixels are dead, and its last block computes the live quarter only
        (Bottleneck.close_sampled).  Few-row split-K (native.fewrow_split) picks its K slices by the row count, so the
        compact 3x3 would sum in another order than the full one: full resolution there."""
        if self.with_gn:   # a group's statistics need every pixel: the stages of a GroupNorm net run at full resolution
            return False
        if not self.skip_dead_pixels or i + 1 >= len(self.res_layers) or i in self.out_indices or native.fewrow_enabled():
            return False
        blocks, nxt = getattr(self, self.res_layers[i]), getattr(self, self.res_layers[i + 1])[0]
        last, ds = blocks[-1], nxt.downsample
        if len(blocks) < 2 or last.downsample is not None or last.stride != 1 or last.with_dcn or last.groups > 1 \
                or any(b.with_gcb or b.with_gen_attention for b in blocks):
            # (a grouped stage runs at full resolution: its compact forms are not built; a context block needs every pixel, and a generalized
            # attention block needs conv2 at every pixel)
            return False
        return (nxt.style == 'caffe' and nxt.conv1_stride == 2 and nxt.conv2_stride == 1 and nxt.conv1.kernel_size == (1, 1)
                and ds is not None and ds[0].kernel_size == (1, 1) and ds[0].stride == (2, 2))

    def _stem(self, x, p):
        """conv1 7x7/2 + bn1 + relu + maxpool 3x3/2 of x [B,3,H,W] -> physical NHWC in the compute dtype.  forward_train_nhwc never reaches
        the split-half branch of the generic route (training runs f32 or bf16)."""
        dt = self.compute_dtype
        if self.with_gn:
            # conv1 raw by the patch-matrix GEMM -> u (split half: f32), gn1 + ReLU in place, the pool
            cols, OH, OW = native.im2col_stem(x.contiguous().float(), dt, STEM_KP)
            u = native.gemm(cols, p['stem'][0], None, relu=False, out_f32=dt == native.SPLIT).view(x.shape[0], OH, OW, 64)
            y = native.group_norm(u, p['gn'][0], p['gn'][1], self.num_groups, self.gn_eps, relu=True, out=u)
            return native.cast(native.maxpool3x3s2_nhwc(y), dt)
        if dt in native.FUSED_DTYPES and self.fused_stem:
            return native.stem_fused(x.contiguous().float(), p['fused'], p['fused_bias'])
        # generic route (f32 / split-half modes): patch matrix + GEMM + pooling
        cols, OH, OW = native.im2col_stem(x.contiguous().float(), dt, STEM_KP)
        # split half is pooled in f32 (max does not act per half plane): the GEMM hands its f32 tile over directly; the cast is a no-op otherwise
        y = native.gemm(cols, p['stem'][0], p['stem'][1], relu=True, out_f32=dt == native.SPLIT).view(x.shape[0], OH, OW, 64)
        return native.cast(native.maxpool3x3s2_nhwc(y), dt)

    def forward(self, x, out=None):
        """x [B,3,H,W] f32 -> tuple of logical-NCHW feature maps (resnet.py:522-533).  out: a contiguous NHWC tensor of
        out_shape_nhwc(...) in the compute dtype that receives the (single) returned map, e.g. a slice of a larger batch."""
        if not x.is_cuda:
            raise NotImplementedError('ResNet runs on the GPU only (no CPU fallback)')
        y = self._stem(x, self.packed(x.device))
        outs, compact = [], False   # compact: y holds every second pixel of every second row of the previous stage's output
        assert out is None or len(self.out_indices) == 1, 'out= needs a single returned map'
        for i, name in enumerate(self.res_layers):
            blocks = list(getattr(self, name))
            route = self.stage_route(i, y.shape[0], y.shape[1], y.shape[2], self.compute_dtype, compact)
            h1 = None
            for j, (blk, step) in enumerate(zip(blocks, route.steps)):
                assert step.h1_in == (h1 is not None), (i, j, step)
                first = compact and j == 0
                if step.compact:
                    y, h1 = blk.close_compact(y, h1, plain=step.kind == 'conv'), None
                elif step.kind == 'close_sampled':
                    y, h1 = blk.close_sampled(y, h1, step.stride), None
                elif step.kind == 'tail_next_live':
                    y, h1 = blk.close_next_live(y, blk.body(y, h1), blocks[j + 1])
                elif step.kind == 'tail_next':   # the next block's conv1 rides on this block's close
                    y, h1 = blk.close_next(y, blk.body(y, h1, first), blocks[j + 1], step, first)
                else:
                    dst = out if out is not None and i == self.out_indices[0] and j + 1 == len(blocks) else None
                    y, h1 = blk.close(y, blk.body(y, h1, first), step, dst, first), None
            compact = route.compact
            if i in self.out_indices:
                outs.append(as_logical(y))
            if out is not None and i == self.out_indices[0]:
                break
        return tuple(outs)

    def forward_train_nhwc(self, x):
        """Training forward in the compute dtype (f32 = parity mode, bf16 = throughput mode with f32 master weights): the
        frozen stem and stages (`frozen_stages`, BatchNorm everywhere) run the inference kernels without a graph, the remaining stages are autograd graphs of HIP convs (Bottleneck.forward_train_nhwc).
        -> the last out_indices map, physical NHWC."""
        if self.gen_attention is not None:
            raise NotImplementedError('a ResNet with generalized attention blocks is inference only: the attention core has no backward')
        if self.with_gn:
            raise NotImplementedError('a ResNet under GroupNorm is inference only: group normalisation has no backward')
        with torch.no_grad():
            y = self._stem(x, self.packed(x.device))
            for i, name in enumerate(self.res_layers):
                if i + 1 <= self.frozen_stages:
                    for blk in getattr(self, name):
                        y = blk.forward_nhwc(y)
        for i, name in enumerate(self.res_layers):
            if i + 1 > self.frozen_stages:
                for blk in getattr(self, name):
                    y = blk.forward_train_nhwc(y)
        return y

    def train(self, mode=True):
        super(ResNet, self).train(False)  # BatchNorm stays in eval mode (norm_eval=True); forward_train_* build the graphs
        return self


@SHARED_HEADS.register_module
class ResLayer(nn.Module, PackedMixin):
    """res5 applied to the whole stride-16 map + the 1x1 2048->256 `new_layer_1` (res_layer.py:16-52,67-74)."""

    def __init__(self, depth, stage=3, stride=2, dilation=1, style='pytorch', norm_cfg=dict(type='BN', requires_grad=True),
                 norm_eval=True, with_cp=False, external_conv=False, dcn=None):
        super(ResLayer, self).__init__()
        self.dcn = dcn
        self.with_gn = norm_kind(norm_cfg, type(self).__name__)[0] == 'GN'
        if self.with_gn and dcn is not None:
            raise NotImplementedError('dcn together with GroupNorm (norm_cfg type GN) is not built')
        if self.with_gn and self._block_kwargs.get('groups', 1) > 1:
            raise NotImplementedError('GroupNorm (norm_cfg type GN) on %s with groups=%d is not built' % (type(self).__name__, self._block_kwargs['groups']))
        self.norm_eval, self.norm_cfg, self.stage, self.external_conv = norm_eval, norm_cfg, stage, external_conv
        self.fp16_enabled = False
        stage_block = ARCH_SETTINGS[depth][stage]
        planes = 64 * 2 ** stage
        inplanes = 64 * 2 ** (stage - 1) * Bottleneck.expansion
        self.add_module('layer{}'.format(stage + 1),
                        make_res_layer(Bottleneck, inplanes, planes, stage_block, stride=stride, dilation=dilation, style=style,
                                       norm_cfg=norm_cfg, dcn=dcn, **self._block_kwargs))
        if external_conv:
            # ConvModule(2048, 256, 1): conv + bias + ReLU, parameters under new_layer_1.conv.*
            self.new_layer_1 = nn.Module()
            self.new_layer_1.conv = nn.Conv2d(2048, 256, 1)
        _freeze(self)
        self._init_packed()

    _block_kwargs = {}   # what every block gets beyond the reference ResLayer's arguments (ResXLayer: groups, base_width)

    def init_weights(self, pretrained=None):
        if pretrained is not None:
            raise NotImplementedError('load checkpoints with load_state_dict (keys match the reference)')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        set_compute_dtype(self, self.compute_dtype)

    def _pack(self, dtype):
        if not self.external_conv:
            return {}
        return dict(ext=fold_conv_bn(self.new_layer_1.conv, None, dtype))

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError('ResLayer runs on the GPU only (no CPU fallback)')
        y = as_nhwc(x, self.compute_dtype)
        for blk in getattr(self, 'layer{}'.format(self.stage + 1)):
            y = blk.forward_nhwc(y)
        if self.external_conv:
            w, b = self.packed(x.device)['ext']
            y = native.conv2d_nhwc(y, w, b, relu=True)
        return as_logical(y)

    def forward_train_nhwc(self, y):
        """res5 + the external 1x1 conv as an autograd graph of HIP convs (f32, physical NHWC in and out)."""
        if self.with_gn:
            raise NotImplementedError('a ResLayer under GroupNorm is inference only: group normalisation has no backward')
        from . import train_ops as TO
        for blk in getattr(self, 'layer{}'.format(self.stage + 1)):
            y = blk.forward_train_nhwc(y)
        if self.external_conv:
            y = TO.conv_bias(y, self.new_layer_1.conv, relu=True)
        return y

    def train(self, mode=True):
        super(ResLayer, self).train(False)
        return self


@BACKBONES.register_module
class ResNeXt(ResNet):
    """mmdet/models/backbones/resnext.py:157-238: a ResNet whose Bottlenecks run conv1 / conv2 / conv3 at
    width = floor(planes * base_width / 64) * groups channels with a grouped 3x3 (native.conv3x3_grouped).  groups == 1 is the ResNet.
    Inference only; dcn is refused on grouped blocks; the grouped stages run at full resolution (no dead-pixel compaction)."""
    arch_settings = dict(ResNet.arch_settings)

    def __init__(self, groups=1, base_width=4, **kwargs):
        self.groups, self.base_width = groups, base_width   # (plain attributes: nn.Module takes them ahead of its own __init__)
        self._block_kwargs = dict(groups=groups, base_width=base_width) if groups != 1 else {}
        if kwargs.get('gen_attention') is not None:
            raise NotImplementedError('gen_attention on ResNeXt is not built: the reference\'s resnext.py accepts the argument and silently drops it')
        super(ResNeXt, self).__init__(**kwargs)


@SHARED_HEADS.register_module
class ResXLayer(ResLayer):
    """mmdet/models/shared_heads/resx_layer.py:15-57: ResLayer on grouped Bottlenecks, with the same hard-wired 2048 -> 256 `new_layer_1`."""

    def __init__(self, depth, stage=3, stride=2, dilation=1, groups=1, base_width=4, style='pytorch', norm_cfg=dict(type='BN', requires_grad=True),
                 norm_eval=True, with_cp=False, external_conv=False, dcn=None):
        self.groups, self.base_width = groups, base_width   # (plain attributes: nn.Module takes them ahead of its own __init__)
        self._block_kwargs = dict(groups=groups, base_width=base_width) if groups != 1 else {}
        super(ResXLayer, self).__init__(depth, stage=stage, stride=stride, dilation=dilation, style=style, norm_cfg=norm_cfg, norm_eval=norm_eval,
                                        with_cp=with_cp, external_conv=external_conv, dcn=dcn)

    def forward_train_nhwc(self, y):
        if self.groups > 1:
            raise NotImplementedError('ResXLayer with groups > 1 is inference only: the grouped 3x3 conv has no backward')
        return super(ResXLayer, self).forward_train_nhwc(y)


# ---- Res2Net (mmdet/models/backbones/res2net_v1b.py) and its shared head (mmdet/models/shared_heads/res2_layer.py)
def _scatter_slices(t, dim, width, wp, scale):
    """t with `scale` slices of `width` along dim -> the same slices at pitch wp, exact zeros in between (the padded-slice layout)."""
    shape = list(t.shape)
    shape[dim] = scale * wp
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    for i in range(scale):
        out.narrow(dim, i * wp, width).copy_(t.narrow(dim, i * width, width))
    return out


class Bottle2neck(nn.Module, PackedMixin):
    """res2net_v1b.py:22-100: conv1 1x1 -> `scale` slices of `width` channels; slice i < scale - 1 goes through its own 3x3
    (+ the previous branch's output in a 'normal' block), the last slice is carried across (through a 3x3 average pool in a 'stage'
    block); conv3 1x1 + shortcut + ReLU.  Inference only.
    On the device the slices live at pitch Wp = width rounded up to 32 in one NHWC map of scale * Wp channels, the pad channels held at
    exact zero by the packed weights (zero rows of conv1 and of the branch weights, zero bias, zero columns of the branch weights and
    of conv3): every sum is the reference's with exact zeros added."""
    expansion = 4
    branch_route = None   # the branch convs: None = native.res2_conv3x3 chooses by shape; 'kernel' / 'composite' force one (tests, tools)

    def __init__(self, inplanes, planes, stride=1, downsample=None, baseWidth=26, scale=4, stype='normal', dilation=1, eps=1e-5):
        super(Bottle2neck, self).__init__()
        if scale == 1:
            raise NotImplementedError('Bottle2neck with scale == 1 (one 3x3 over the whole width, nothing carried) is not built')
        assert stype in ('normal', 'stage'), stype
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        width = int(math.floor(planes * (baseWidth / 64.0)))
        self.conv1 = nn.Conv2d(inplanes, width * scale, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width * scale, eps=eps)
        self.nums = scale - 1
        if stype == 'stage':
            self.pool = nn.AvgPool2d(kernel_size=3, stride=stride, padding=1)
        self.convs = nn.ModuleList([nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
                                    for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm2d(width, eps=eps) for _ in range(self.nums)])
        self.conv3 = nn.Conv2d(width * scale, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion, eps=eps)
        self.downsample = downsample
        self.stype, self.scale, self.width = stype, scale, width
        self.wp = native.res2_pad_width(width)
        self._init_packed()

    def _pack(self, dtype):
        width, wp, scale = self.width, self.wp, self.scale
        w1, b1 = fold_conv_bn(self.conv1, self.bn1, torch.float32)
        p = dict(c1=(native.as_operand(_scatter_slices(w1, 0, width, wp, scale), dtype), _scatter_slices(b1, 0, width, wp, scale).contiguous()))
        p['br'] = []
        for conv, bn in zip(self.convs, self.bns):
            w, b = fold_conv_bn(conv, bn, torch.float32)
            wpad = torch.zeros((wp, 3, 3, wp), dtype=torch.float32, device=w.device)
            bpad = torch.zeros((wp,), dtype=torch.float32, device=w.device)
            wpad[:width, :, :, :width], bpad[:width] = w, b
            p['br'].append((native.Res2Weight(wpad, dtype), bpad))
        w3, b3 = fold_conv_bn(self.conv3, self.bn3, torch.float32)
        p['c3'] = (native.as_operand(_scatter_slices(w3, 3, width, wp, scale), dtype), b3)
        if self.downsample is not None:
            p['ds'] = fold_conv_bn(self.downsample[1], self.downsample[2], dtype)
        return p

    def forward_nhwc(self, x, out=None):
        """x [B,H,W,inplanes] physical NHWC in the compute format -> [B,OH,OW,4*planes]; out as in Bottleneck.close."""
        p = self.packed(x.device)
        wp, s = self.wp, self.stride
        P = native.conv2d_nhwc(x, p['c1'][0], p['c1'][1], relu=True)
        B, H, W, _ = P.shape
        Q = torch.empty((B, (H - 1) // s + 1, (W - 1) // s + 1, self.scale * wp), dtype=P.dtype, device=P.device)
        for i, (w, b) in enumerate(p['br']):
            prev = self.stype == 'normal' and i > 0   # res2net_v1b.py:76-79: sp + spx[i], sp being the branch before
            native.res2_conv3x3(P, i * wp, w, b, add=Q if prev else None, add_off=(i - 1) * wp if prev else 0, out=Q, out_off=i * wp, stride=s,
                                dil=self.dilation, relu=True, route=self.branch_route)
        if self.stype == 'stage':   # AvgPool2d(3, stride, padding=1): count_include_pad, always / 9
            native.avgpool_nhwc(P, 3, s, 1, False, True, x_off=self.nums * wp, C=wp, out=Q, out_off=self.nums * wp)
        else:
            native.avgpool_nhwc(P, 1, 1, 0, False, True, x_off=self.nums * wp, C=wp, out=Q, out_off=self.nums * wp)
        identity = x
        if self.downsample is not None:
            k = self.downsample[0].kernel_size
            xi = x if k == 1 else native.avgpool_nhwc(x, k, k, 0, True, False)   # (a 1 x 1 pool at stride 1 is the identity)
            identity = native.conv2d_nhwc(xi, p['ds'][0], p['ds'][1], relu=False)
        return native.conv2d_nhwc(Q, p['c3'][0], p['c3'][1], resid=identity, relu=True, out=out)

    def forward(self, x):
        return as_logical(self.forward_nhwc(as_nhwc(x, self.compute_dtype)))

    def forward_train_nhwc(self, x):
        raise NotImplementedError('Bottle2neck is inference only: the slice conv and the pitched pool have no backward')


def make_res2_layer(block, inplanes, planes, blocks, baseWidth, scale, stride=1, dilation=1, eps=1e-5):
    """res2net_v1b.py:103-122.  The first block is the 'stage' block: it takes the stride and NOT the dilation; the others are 'normal' at
    `dilation`.  The shortcut is AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False) -> 1x1 conv -> BN."""
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(nn.AvgPool2d(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False),
                                   nn.Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=1, bias=False),
                                   nn.BatchNorm2d(planes * block.expansion, eps=eps))
    layers = [block(inplanes, planes, stride, downsample=downsample, stype='stage', baseWidth=baseWidth, scale=scale, eps=eps)]
    inplanes = planes * block.expansion
    for _ in range(1, blocks):
        layers.append(block(inplanes, planes, baseWidth=baseWidth, scale=scale, dilation=dilation, eps=eps))
    return nn.Sequential(*layers)


def _res2_refuse(conv_cfg, norm_cfg, dcn, gcb=None, gen_attention=None):
    if dcn is not None or gcb is not None or gen_attention is not None or conv_cfg is not None:
        raise NotImplementedError('dcn / gcb / gen_attention / conv_cfg are not built for Res2Net (the reference accepts and ignores them)')
    if (norm_cfg or {}).get('type', 'BN') != 'BN':
        raise NotImplementedError('only frozen BatchNorm is supported')


@BACKBONES.register_module
class Res2Net(nn.Module, PackedMixin):
    """res2net_v1b.py:125-271: Res2Net-101 v1b, 26w x 4s, hard-wired -- layers (3, 4, 23, 3), a deep stem of three 3x3 convs, three
    stages at strides (1, 2, 2) and dilation 1 -- returning ONE map: 1024 channels at stride 16.  The reference ignores strides,
    dilations, num_stages and out_indices beyond their assertions; arguments it would silently disobey are refused here."""
    arch_settings = {101: (Bottle2neck, (3, 4, 23, 3))}

    def __init__(self, in_channels=3, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch',
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), gcb=None, stage_with_gcb=(False, False, False, False), gen_attention=None,
                 stage_with_gen_attention=((), (), (), ()), with_cp=False, zero_init_residual=True):
        super(Res2Net, self).__init__()
        _res2_refuse(conv_cfg, norm_cfg, dcn, gcb, gen_attention)
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        assert in_channels == 3
        if tuple(strides[:3]) != (1, 2, 2)[:num_stages] or any(d != 1 for d in dilations):
            raise ValueError('Res2Net runs three stages at strides (1, 2, 2) and dilation 1 whatever it is given (res2net_v1b.py:188-195): '
                             'strides=%r dilations=%r would be ignored' % (tuple(strides), tuple(dilations)))
        self.num_stages, self.strides, self.dilations, self.out_indices = num_stages, strides, dilations, out_indices
        self.frozen_stages, self.norm_eval, self.style = frozen_stages, norm_eval, style
        self.baseWidth, self.scale = 26, 4
        block, layers = self.arch_settings[101]
        eps = norm_cfg.get('eps', 1e-5)
        self.conv1 = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32, eps=eps), nn.ReLU(inplace=True),
                                   nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32, eps=eps), nn.ReLU(inplace=True),
                                   nn.Conv2d(32, 64, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(64, eps=eps)
        self.layer1 = make_res2_layer(block, 64, 64, layers[0], baseWidth=self.baseWidth, scale=self.scale, eps=eps)
        self.layer2 = make_res2_layer(block, 256, 128, layers[1], stride=2, baseWidth=self.baseWidth, scale=self.scale, eps=eps)
        self.layer3 = make_res2_layer(block, 512, 256, layers[2], stride=2, baseWidth=self.baseWidth, scale=self.scale, eps=eps)
        self.res_layers = ['layer1', 'layer2', 'layer3']
        self.feat_dim = 1024
        _freeze(self)
        self._init_packed()

    def init_weights(self, pretrained=None):
        """res2net_v1b.py:220-232 (pretrained checkpoints are loaded by the caller via load_state_dict)."""
        if pretrained is not None:
            raise NotImplementedError('load checkpoints with load_state_dict (keys match the reference)')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        set_compute_dtype(self, self.compute_dtype)

    @staticmethod
    def stem_channels(dtype):
        """Channels of the two 32-channel stem maps on the device: 32 zero-padded to the Cin multiple conv2d_nhwc asks of the mode."""
        return 64 if dtype in (torch.bfloat16, torch.float16) else 32

    def _pack(self, dtype):
        cp = self.stem_channels(dtype)
        w0, b0 = fold_conv_bn(self.conv1[0], self.conv1[1], torch.float32)    # [32,3,3,3]: stays f32 (native.stem3x3s2_first)
        w1, b1 = fold_conv_bn(self.conv1[3], self.conv1[4], torch.float32)    # [32,3,3,32] -> zero rows and columns up to cp
        w2, b2 = fold_conv_bn(self.conv1[6], self.bn1, torch.float32)         # [64,3,3,32] -> zero columns up to cp
        w1p = torch.zeros((cp, 3, 3, cp), dtype=torch.float32, device=w1.device)
        b1p = torch.zeros((cp,), dtype=torch.float32, device=w1.device)
        w1p[:32, :, :, :32], b1p[:32] = w1, b1
        w2p = torch.zeros((64, 3, 3, cp), dtype=torch.float32, device=w2.device)
        w2p[:, :, :, :32] = w2
        return dict(s0=(w0.contiguous(), b0.contiguous()), s1=(native.as_operand(w1p, dtype), b1p), s2=(native.as_operand(w2p, dtype), b2.contiguous()))

    def out_shape_nhwc(self, B, H, W):
        """Physical [B,h,w,1024] shape of the returned map for a [B,3,H,W] input: stem 3x3/2 + pool 3x3/2, then strides 1, 2, 2."""
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        for _ in range(2):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return (B, h, w, 1024)

    def _stem(self, x, p):
        """conv1 (three 3x3 convs) + bn1 + ReLU + maxpool 3x3/2 of x [B,3,H,W] -> physical NHWC [B,h,w,64] in the compute format."""
        dt = self.compute_dtype
        y = native.stem3x3s2_first(x.contiguous().float(), p['s0'][0], p['s0'][1], dt, channels=self.stem_channels(dt))
        y = native.conv2d_nhwc(y, p['s1'][0], p['s1'][1], relu=True, pad=1)
        y = native.conv2d_nhwc(y, p['s2'][0], p['s2'][1], relu=True, pad=1)
        return native.maxpool3x3s2_nhwc(y)

    def forward(self, x, out=None):
        """x [B,3,H,W] f32 -> a tuple of ONE logical-NCHW map (res2net_v1b.py:247-262).  out: a contiguous NHWC tensor of
        out_shape_nhwc(...) in the compute dtype that receives it, e.g. a slice of a larger batch."""
        if not x.is_cuda:
            raise NotImplementedError('Res2Net runs on the GPU only (no CPU fallback)')
        y = self._stem(x, self.packed(x.device))
        for i, name in enumerate(self.res_layers):
            blocks = list(getattr(self, name))
            for j, blk in enumerate(blocks):
                y = blk.forward_nhwc(y, out if i + 1 == len(self.res_layers) and j + 1 == len(blocks) else None)
        return (as_logical(y),)

    def forward_train_nhwc(self, x):
        raise NotImplementedError('Res2Net is inference only: the slice conv and the pitched pool have no backward')

    def train(self, mode=True):
        super(Res2Net, self).train(False)
        return self


@SHARED_HEADS.register_module
class Res2Layer(nn.Module, PackedMixin):
    """res2_layer.py:13-81: layer{stage+1} of Res2Net-101 on Bottle2necks (26w x 4s) + the hard-wired 1x1 2048 -> 256 `new_layer_1`.
    The C5 form is stride=1, dilation=2: the first block at dilation 1 with a 3x3/1 pool, the other two at dilation 2."""

    def __init__(self, depth, stage=3, stride=2, dilation=1, style='pytorch', norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True,
                 with_cp=False, external_conv=False, dcn=None):
        super(Res2Layer, self).__init__()
        _res2_refuse(None, norm_cfg, dcn)
        self.norm_eval, self.norm_cfg, self.stage, self.external_conv = norm_eval, norm_cfg, stage, external_conv
        self.fp16_enabled = False
        block, stage_blocks = Res2Net.arch_settings[depth]   # (KeyError for any depth but 101, as in the reference)
        planes = 64 * 2 ** stage
        inplanes = 64 * 2 ** (stage - 1) * block.expansion
        self.add_module('layer{}'.format(stage + 1), make_res2_layer(block, inplanes, planes, stage_blocks[stage], baseWidth=26, scale=4, stride=stride,
                                                                      dilation=dilation, eps=norm_cfg.get('eps', 1e-5)))
        if external_conv:
            self.new_layer_1 = nn.Module()   # ConvModule(2048, 256, 1): conv + bias + ReLU, parameters under new_layer_1.conv.*
            self.new_layer_1.conv = nn.Conv2d(2048, 256, 1)
        _freeze(self)
        self._init_packed()

    init_weights = ResLayer.init_weights
    _pack = ResLayer._pack
    forward = ResLayer.forward

    def forward_train_nhwc(self, y):
        raise NotImplementedError('Res2Layer is inference only: the slice conv and the pitched pool have no backward')

    def train(self, mode=True):
        super(Res2Layer, self).train(False)
        return self
