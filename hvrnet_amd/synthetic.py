"""Seeded synthetic weights and frames for benchmarks, smoke and parity runs.

There is no network for datasets or checkpoints, so the benchmark uses random-init weights
of the reference architecture and synthetic frames of the reference's input shape
(SURVEY.md 8(d)).  Everything is generated on the CPU torch generator so that the GPU path,
the CPU oracle and the golden-vector script (which feeds the same tensors to the reference's
own modules) see bit-identical tensors.

State-dict keys and shapes are the reference's checkpoint contract:
  backbone.*      mmdet/models/backbones/resnet.py:456-466,269-329 (R101, 3 stages, caffe)
  shared_head.*   mmdet/models/shared_heads/res_layer.py:37-52
  rpn_head.*      mmdet/models/anchor_heads/rpn_head.py:18-23 (synth_ga_rpn_state_dict: ga_rpn_head.py:19-22, guided_anchor_head.py:172-185)
  bbox_head.*     mmdet/models/bbox_heads/selsa_bbox_head.py:45-89, hrnmp_bbox_head.py:121-189

The reference's own init (`zero_init_residual=True`, resnet.py:513-518; N(0, 0.01) head linears)
makes random-init parity degenerate (dead residual branches, uniform attention rows), so the BN
statistics are randomised and the head weights are scaled up; the scales below were chosen so
that RPN scores, attention rows and class scores are all well away from uniform/saturated.
"""
import math

import torch

STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}

# multipliers on the reference's N(0, 0.01) init
NEW_LAYER_GAIN = 0.0125  # shared_head.new_layer_1: brings RoI features to unit scale
HEAD_FC1_GAIN = 1.0      # fc_new_1 (12544 inputs)
HEAD_FCK_GAIN = 3.0      # fc_new_2..4 (1024 inputs)
HEAD_QK_GAIN = 8.0      # q / k projections: attention logit std ~3 (peaky rows, not one-hot)
HEAD_OUT_GAIN = 3.0      # linear_out_k (1x1 conv): relation update comparable to the residual
HEAD_CLS_GAIN = 7.0      # fc_cls: spreads class scores
HEAD_REG_GAIN = 3.5
RPN_CONV_GAIN = 1.0
RPN_CLS_GAIN = 0.3
RPN_REG_GAIN = 0.07
# GA-RPN (synth_ga_rpn_state_dict): on the synthetic frames the C4 map is ~unit scale, so the 3x3 conv's output has a std of about
# 0.01 * sqrt(9 C) * gain.  The location logits are centred on logit(loc_filter_thr) so that about half the pixels are kept; the
# shape deltas stay within a few units, far inside the +-13.8 (= |log 1e-6|) clip after the anchoring stds (0.07 / 0.14).
GA_CONV_GAIN = 3.0     # rpn_conv with zero-sum kernels (see synth_ga_rpn_state_dict): contrast is a fraction of the level
GA_LOC_GAIN = 3.0
GA_SHAPE_GAIN = 3.0
GA_OFFSET_STD = 0.1     # feature_adaption.conv_offset: the reference's own init
GA_ADAPT_GAIN = 1.0


def _conv(g, cout, cin, k):
    std = math.sqrt(2.0 / (cout * k * k))  # kaiming_normal_, mode='fan_out', relu (mmcv kaiming_init)
    return torch.randn((cout, cin, k, k), generator=g) * std


def _bn(g, sd, prefix, c, gamma_scale=1.0):
    sd[prefix + '.weight'] = (torch.rand(c, generator=g) + 0.5) * gamma_scale
    sd[prefix + '.bias'] = torch.randn(c, generator=g) * 0.1
    sd[prefix + '.running_mean'] = torch.randn(c, generator=g) * 0.1
    sd[prefix + '.running_var'] = torch.rand(c, generator=g) + 0.5
    sd[prefix + '.num_batches_tracked'] = torch.zeros((), dtype=torch.long)


def _gn(g, sd, prefix, c, gamma_scale=1.0):
    """Keys of an nn.GroupNorm (no running statistics): gamma ~ U(0.5, 1.5), beta ~ 0.1 N."""
    sd[prefix + '.weight'] = (torch.rand(c, generator=g) + 0.5) * gamma_scale
    sd[prefix + '.bias'] = torch.randn(c, generator=g) * 0.1


def _norm(g, sd, prefix, c, norm, gamma_scale=1.0):
    """The norm layer behind a conv under the reference's name: prefix names the BatchNorm ('....bn1'); a GroupNorm is 'gn' + the same
    postfix (norm.py: abbreviation + postfix), a module inside an nn.Sequential ('downsample.1') keeps its index."""
    if norm == 'GN':
        head, _, last = prefix.rpartition('.')
        return _gn(g, sd, head + '.' + ('gn' + last[2:] if last.startswith('bn') else last), c, gamma_scale)
    return _bn(g, sd, prefix, c, gamma_scale)


def _gcb(g, sd, prefix, c, ratio, pooling_type='att', fusion_types=('channel_add', )):
    """Keys of a ContextBlock (context_block.py:31-51).  The reference zeroes the last conv of each branch, which makes a fresh block the
    identity (channel_add) or a constant 1/2 (channel_mul): here it gets values, so that the block shows in the output."""
    r = int(c * ratio)
    if pooling_type == 'att':
        sd[prefix + '.conv_mask.weight'] = torch.randn((1, c, 1, 1), generator=g) * math.sqrt(2.0 / c)
        sd[prefix + '.conv_mask.bias'] = torch.randn(1, generator=g) * 0.1
    for name in ('channel_add', 'channel_mul'):   # (the reference registers add first)
        if name in fusion_types:
            q = '%s.%s_conv' % (prefix, name)
            sd[q + '.0.weight'] = torch.randn((r, c, 1, 1), generator=g) * math.sqrt(2.0 / c)
            sd[q + '.0.bias'] = torch.randn(r, generator=g) * 0.1
            sd[q + '.1.weight'] = (torch.rand(r, generator=g) + 0.5).view(r, 1, 1)
            sd[q + '.1.bias'] = (torch.randn(r, generator=g) * 0.1).view(r, 1, 1)
            sd[q + '.3.weight'] = torch.randn((c, r, 1, 1), generator=g) * (0.25 * math.sqrt(1.0 / r))
            sd[q + '.3.bias'] = torch.randn(c, generator=g) * 0.05


def _gen_attention(g, sd, prefix, c, num_heads=9, position_embedding_dim=-1, attention_type='1111', **_shape_free):
    """Keys of a GeneralizedAttention block (generalized_attention.py:60-109) in the reference's order.  The reference starts gamma at 0,
    which makes a fresh block the identity: here gamma, the biases and proj_conv's bias get values, so that the block shows in the output.
    The projections are scaled so that the energies of a unit-scale map spread over a few units (peaky rows, not one-hot)."""
    t = [bool(int(b)) for b in attention_type]
    d = c // num_heads
    oc, f = d * num_heads, (position_embedding_dim if position_embedding_dim > 0 else c) // 2

    def u(shape, fan_in, gain=1.0):   # kaiming-uniform, a = 1
        return (torch.rand(shape, generator=g) * 2.0 - 1.0) * (gain * math.sqrt(3.0 / fan_in))
    if t[0] or t[1]:
        sd[prefix + '.query_conv.weight'] = u((oc, c, 1, 1), c, 1.5)
    if t[0] or t[2]:
        sd[prefix + '.key_conv.weight'] = u((oc, c, 1, 1), c, 1.5)
    sd[prefix + '.value_conv.weight'] = u((oc, c, 1, 1), c)
    if t[1] or t[3]:
        sd[prefix + '.appr_geom_fc_x.weight'] = u((oc, f), f)
        sd[prefix + '.appr_geom_fc_y.weight'] = u((oc, f), f)
    sd[prefix + '.proj_conv.weight'] = u((c, oc, 1, 1), oc)
    sd[prefix + '.proj_conv.bias'] = torch.randn(c, generator=g) * 0.05
    sd[prefix + '.gamma'] = torch.rand(1, generator=g) * 0.5 + 0.5
    # (parameters registered with nn.Parameter come first in a state dict, the sub-modules' behind them: state_dict() order is not asserted
    # by load_state_dict, the key SET is)
    stdv = 1.0 / math.sqrt(2 * d)
    if t[2]:
        sd[prefix + '.appr_bias'] = (torch.rand(oc, generator=g) * 2.0 - 1.0) * stdv
    if t[3]:
        sd[prefix + '.geom_bias'] = (torch.rand(oc, generator=g) * 2.0 - 1.0) * stdv


def _res_layer(g, sd, prefix, inplanes, planes, blocks, groups=1, base_width=4, gcb=None, gen_attention=None, gen_attention_blocks=(),
               norm='BN'):
    width = planes if groups == 1 else int(math.floor(planes * (base_width / 64))) * groups   # resnext.py:21-24
    for i in range(blocks):
        p = '%s.%d' % (prefix, i)
        cin = inplanes if i == 0 else planes * 4
        sd[p + '.conv1.weight'] = _conv(g, width, cin, 1)
        _norm(g, sd, p + '.bn1', width, norm)
        sd[p + '.conv2.weight'] = _conv(g, width, width // groups, 3) * math.sqrt(groups)   # (fan_out counts one group's inputs: keep the output's scale)
        _norm(g, sd, p + '.bn2', width, norm)
        sd[p + '.conv3.weight'] = _conv(g, planes * 4, width, 1)
        # a live but damped residual branch keeps 33 stacked blocks from blowing up
        _norm(g, sd, p + '.bn3', planes * 4, norm, gamma_scale=0.25)
        if i == 0:
            sd[p + '.downsample.0.weight'] = _conv(g, planes * 4, cin, 1)
            _norm(g, sd, p + '.downsample.1', planes * 4, norm)
        if gcb is not None:
            _gcb(g, sd, p + '.context_block', planes * 4, **gcb)
        if gen_attention is not None and i in gen_attention_blocks:
            _gen_attention(g, sd, p + '.gen_attention_block', planes, **gen_attention)


def _res2_layer(g, sd, prefix, inplanes, planes, blocks, base_width=26, scale=4):
    """Keys of make_res2_layer (res2net_v1b.py:103-122) in the reference's order: conv1, bn1, convs, bns, conv3, bn3, then the
    pool -> 1x1 -> BN shortcut of the first block under downsample.1 / downsample.2 (the pool is downsample.0)."""
    width = int(math.floor(planes * (base_width / 64.0)))
    for i in range(blocks):
        p = '%s.%d' % (prefix, i)
        cin = inplanes if i == 0 else planes * 4
        sd[p + '.conv1.weight'] = _conv(g, width * scale, cin, 1)
        _bn(g, sd, p + '.bn1', width * scale)
        for j in range(scale - 1):
            sd[p + '.convs.%d.weight' % j] = _conv(g, width, width, 3)
        for j in range(scale - 1):
            _bn(g, sd, p + '.bns.%d' % j, width)
        sd[p + '.conv3.weight'] = _conv(g, planes * 4, width * scale, 1)
        _bn(g, sd, p + '.bn3', planes * 4, gamma_scale=0.25)
        if i == 0:
            sd[p + '.downsample.1.weight'] = _conv(g, planes * 4, cin, 1)
            _bn(g, sd, p + '.downsample.2', planes * 4)


def _linear(g, sd, prefix, cout, cin, gain, conv=False):
    w = torch.randn((cout, cin), generator=g) * (0.01 * gain)
    sd[prefix + '.weight'] = w.view(cout, cin, 1, 1) if conv else w
    sd[prefix + '.bias'] = torch.randn(cout, generator=g) * 0.01


def synth_state_dict(head='hvr', seed=0, depth=101, num_classes=31, fc_dim=1024, roi_feat=256 * 49, groups=1, base_width=4, arch='resnet',
                     gcb=None, stage_with_gcb=(False, True, True), gen_attention=None, stage_with_gen_attention=((), (), ()), norm='BN'):
    """Full detector state dict (f32, CPU) with the reference's key names.  groups / base_width: a ResNeXt backbone + ResXLayer.
    arch='res2net': a Res2Net backbone (101 layers, 26w x 4s, deep stem) + Res2Layer; the heads' keys are the same.
    gcb: dict(ratio=..., pooling_type=..., fusion_types=...) adds the context-block keys to the backbone stages marked in stage_with_gcb
    (ResNet / ResNeXt), with non-zero last convs; None (the default) leaves every key and value as before.
    gen_attention: the dict ResNet takes adds the keys of a generalized attention block to the blocks stage_with_gen_attention names per
    stage (ResNet), with non-zero gamma and biases; None (the default) leaves every key and value as before.
    norm='GN': the backbone and res5 of norm_cfg=dict(type='GN', ...) -- gn1 / gn2 / gn3 and downsample.1 hold a GroupNorm's weight and bias only
    (plain ResNet); 'BN' (the default) leaves every key and value as before."""
    assert arch in ('resnet', 'res2net'), arch
    assert gcb is None or arch == 'resnet', 'Res2Net takes no context blocks'
    assert gen_attention is None or (arch == 'resnet' and groups == 1), 'only ResNet takes generalized attention blocks'
    assert norm in ('BN', 'GN'), norm
    assert norm == 'BN' or (arch == 'resnet' and groups == 1 and gcb is None and gen_attention is None), 'only the plain ResNet takes GroupNorm'
    g = torch.Generator().manual_seed(seed)
    sd = {}
    blocks = STAGE_BLOCKS[depth]
    if arch == 'res2net':
        assert depth == 101 and groups == 1, 'Res2Net is the 101-layer 26w x 4s net only'
        for idx, (co, ci) in ((0, (32, 3)), (3, (32, 32)), (6, (64, 32))):   # res2net_v1b.py:174-182: conv1.0 / .1 / .3 / .4 / .6
            sd['backbone.conv1.%d.weight' % idx] = _conv(g, co, ci, 3)
            if idx < 6:
                _bn(g, sd, 'backbone.conv1.%d' % (idx + 1), co)
        _bn(g, sd, 'backbone.bn1', 64)
        inplanes = 64
        for i in range(3):
            _res2_layer(g, sd, 'backbone.layer%d' % (i + 1), inplanes, 64 * 2 ** i, blocks[i])
            inplanes = 64 * 2 ** i * 4
        _res2_layer(g, sd, 'shared_head.layer4', 1024, 512, blocks[3])
    else:
        sd['backbone.conv1.weight'] = _conv(g, 64, 3, 7)
        _norm(g, sd, 'backbone.bn1', 64, norm)
        inplanes = 64
        for i in range(3):
            _res_layer(g, sd, 'backbone.layer%d' % (i + 1), inplanes, 64 * 2 ** i, blocks[i], groups, base_width,
                       gcb if gcb is not None and stage_with_gcb[i] else None, gen_attention,
                       tuple(stage_with_gen_attention[i]) if gen_attention is not None and i < len(stage_with_gen_attention) else (), norm)
            inplanes = 64 * 2 ** i * 4
        _res_layer(g, sd, 'shared_head.layer4', 1024, 512, blocks[3], groups, base_width, norm=norm)
    sd['shared_head.new_layer_1.conv.weight'] = _conv(g, 256, 2048, 1) * NEW_LAYER_GAIN
    sd['shared_head.new_layer_1.conv.bias'] = torch.randn(256, generator=g) * 0.01
    # RPN (12 anchors)
    w = torch.randn((512, 1024, 3, 3), generator=g) * (0.01 * RPN_CONV_GAIN)
    sd['rpn_head.rpn_conv.weight'] = w
    sd['rpn_head.rpn_conv.bias'] = torch.zeros(512)
    _linear(g, sd, 'rpn_head.rpn_cls', 12, 512, RPN_CLS_GAIN, conv=True)
    _linear(g, sd, 'rpn_head.rpn_reg', 48, 512, RPN_REG_GAIN, conv=True)
    # relation head
    stages = 4 if head == 'hvr' else 2
    for k in range(1, stages + 1):
        _linear(g, sd, 'bbox_head.fc_new_%d' % k, fc_dim, roi_feat if k == 1 else fc_dim,
                HEAD_FC1_GAIN if k == 1 else HEAD_FCK_GAIN)
        p = 'bbox_head.selsa_%d.' % k
        _linear(g, sd, p + 'q_data_fc_%d' % k, fc_dim, fc_dim, HEAD_QK_GAIN)
        _linear(g, sd, p + 'k_data_fc_%d' % k, fc_dim, fc_dim, HEAD_QK_GAIN)
        _linear(g, sd, p + 'linear_out_%d' % k, fc_dim, fc_dim, HEAD_OUT_GAIN, conv=True)
    _linear(g, sd, 'bbox_head.fc_cls', num_classes, fc_dim, HEAD_CLS_GAIN)
    _linear(g, sd, 'bbox_head.fc_reg', 4, fc_dim, HEAD_REG_GAIN)
    if head == 'hvr':
        _linear(g, sd, 'bbox_head.fc_cls_2', num_classes, fc_dim, HEAD_CLS_GAIN)
        _linear(g, sd, 'bbox_head.fc_reg_2', 4, fc_dim, HEAD_REG_GAIN)
    return sd


def synth_ga_rpn_state_dict(channels=1024, deformable_groups=4, loc_filter_thr=0.01, seed=0, prefix='rpn_head.'):
    """Seeded GARPNHead weights (f32, CPU) under the reference's key names (ga_rpn_head.py:19-22, guided_anchor_head.py:172-185,
    :38-46), in_channels == feat_channels == channels.  A generator of its own: synth_state_dict's keys and values do not change.
    Replace the `rpn_head.*` entries of a detector state dict with these to run a GA-RPN detector."""
    g = torch.Generator().manual_seed(seed * 7919 + 26)
    sd = {}
    # C4 is a post-ReLU map with a large common level, and so is the 3x3 conv's output under zero-mean random weights: a random 1x1
    # head on it sees one offset shared by every pixel, larger than the variation between pixels, and the location mask comes out
    # all-kept or all-dropped whatever the gains.  So every 3x3 kernel here sums to zero over its taps (it answers to the map's spatial
    # contrast, its output channels share one distribution) and the location weights sum to zero over the channels: the location logit
    # then spreads evenly around its bias, which sits on the threshold.
    w = torch.randn((channels, channels, 3, 3), generator=g)
    sd[prefix + 'rpn_conv.weight'] = (w - w.mean(dim=(2, 3), keepdim=True)) * (0.01 * GA_CONV_GAIN)
    sd[prefix + 'rpn_conv.bias'] = torch.zeros(channels)
    _linear(g, sd, prefix + 'conv_loc', 1, channels, GA_LOC_GAIN, conv=True)
    sd[prefix + 'conv_loc.weight'] -= sd[prefix + 'conv_loc.weight'].mean()
    sd[prefix + 'conv_loc.bias'] = torch.full((1,), math.log(loc_filter_thr / (1.0 - loc_filter_thr)))   # half the pixels pass the filter
    _linear(g, sd, prefix + 'conv_shape', 2, channels, GA_SHAPE_GAIN, conv=True)
    sd[prefix + 'feature_adaption.conv_offset.weight'] = torch.randn((deformable_groups * 18, 2, 1, 1), generator=g) * GA_OFFSET_STD
    sd[prefix + 'feature_adaption.conv_adaption.weight'] = torch.randn((channels, channels, 3, 3), generator=g) * (0.01 * GA_ADAPT_GAIN)
    _linear(g, sd, prefix + 'conv_cls', 1, channels, RPN_CLS_GAIN, conv=True)
    _linear(g, sd, prefix + 'conv_reg', 4, channels, RPN_REG_GAIN, conv=True)
    return sd


def synth_frame(index, seed=0, img_hw=(600, 1000), pad_hw=(608, 1008)):
    """One mean-subtracted BGR-scale frame [1,3,pad_h,pad_w] f32 (zero padded, Pad(size_divisor=16))."""
    g = torch.Generator().manual_seed(seed * 100003 + index)
    h, w = img_hw
    # low-frequency content + noise, so RPN / RoI features are not white noise
    coarse = torch.randn((1, 3, h // 40 + 1, w // 40 + 1), generator=g)
    img = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=False) * 40.0
    img = img + torch.randn((1, 3, h, w), generator=g) * 15.0
    out = torch.zeros((1, 3, pad_hw[0], pad_hw[1]))
    out[:, :, :h, :w] = img
    return out


def synth_meta(img_hw=(600, 1000), pad_hw=(608, 1008)):
    return dict(img_shape=(img_hw[0], img_hw[1], 3), ori_shape=(img_hw[0], img_hw[1], 3), pad_shape=(pad_hw[0], pad_hw[1], 3),
                scale_factor=1.0, flip=False)
