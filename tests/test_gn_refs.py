"""CPU checks of the GroupNorm feature: the f64 statement of the rule (tests/gn_refs.py) against torch, its bounds against an f32 emulation
of the stated partial / merge rule and against every stated mistake, and the modules -- ResNet / ResLayer / Bottleneck under
norm_cfg = dict(type='GN', ...) -- against the reference's key lists and float64 blocks (tests/golden/gn_modules.json, g25_gn_block.npz:
make_gn_golden.py), their refusals, their route tables and the synthetic checkpoint."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import hvrnet_amd
from hvrnet_amd import backbone, native, synthetic
from tests import forward_kernel_refs as K
from tests import gn_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GN32 = dict(type='GN', num_groups=32)
CPU_RAGGED = (1, 13, 15, 64, 32)      # 195 pixels: S = 4 runs of 49, the last one holds 48
FAMILIES = ('real', 'offset', 'constant')
MODES = ('f32', 'bf16', 'f16')


def _case(geo, family, mode, seed=0, normalised=True):
    B, H, W, C, G = geo
    P = H * W
    S = R.splits(B, P)[0]
    u = R.operands(family, mode, B, P, C, G, seed)
    resid = R.operands(family if family != 'constant' else 'real', mode, B, P, C, G, seed + 1)
    gamma, beta = R.affine(C, seed + 2)
    rn = R.affine(C, seed + 3) if normalised else None
    return dict(u=u, gamma=gamma, beta=beta, G=G, S=S, resid=resid, resid_norm=rn, relu=True)


def _statement(c, **kw):
    return R.gn_statement(c['u'], c['gamma'], c['beta'], c['G'], R.EPS, c['resid'], c['resid_norm'], c['relu'], S=c['S'], **kw)


def _inside(y, st, mode):
    lo, hi = K.stored_bracket(torch.from_numpy(st['y']), torch.from_numpy(st['bound']), mode)
    y = torch.from_numpy(np.ascontiguousarray(y))
    return bool(((y >= lo) & (y <= hi)).all())


def _store(v, mode):
    return torch.from_numpy(v).float().to(K.STORE[mode]).double().numpy()


@pytest.mark.parametrize('geo', R.GEOMETRIES + (CPU_RAGGED,))
def test_statement_equals_torch_group_norm_in_f64(geo):
    B, H, W, C, G = geo
    c = _case(geo, 'real', 'f32')
    st = R.gn_statement(c['u'], c['gamma'], c['beta'], G)
    x = torch.from_numpy(c['u']).view(B, H * W, C).permute(0, 2, 1)
    want = F.group_norm(x, G, torch.from_numpy(c['gamma']), torch.from_numpy(c['beta']), R.EPS).permute(0, 2, 1).numpy()
    assert np.abs(st['y'] - want).max() <= 1e-12
    full = _statement(c)
    xr = torch.from_numpy(c['resid']).view(B, H * W, C).permute(0, 2, 1)
    r = F.group_norm(xr, G, torch.from_numpy(c['resid_norm'][0]), torch.from_numpy(c['resid_norm'][1]), R.EPS).permute(0, 2, 1).numpy()
    assert np.abs(full['y'] - np.maximum(want + r, 0.0)).max() <= 1e-12


def test_splits_cut_the_ragged_maps_into_several_runs():
    assert R.splits(1, 13 * 15) == (4, 49) and R.splits(1, 129 * 131) == (64, 265) and 129 * 131 - 63 * 265 == 204
    assert R.splits(15, 152 * 252) == (64, 599) and R.splits(512, 38 * 63) == (2, 1197) and R.splits(2, 1) == (1, 1)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('mode', MODES)
def test_f32_emulation_of_the_rule_lies_inside_the_bracket(family, mode):
    for geo in R.GEOMETRIES + (CPU_RAGGED,):
        c = _case(geo, family, mode)
        st = _statement(c)
        for lanes in (1, 4):
            y = R.emulate_f32(c['u'], c['gamma'], c['beta'], c['G'], R.EPS, c['S'], lanes, c['resid'], c['resid_norm'], c['relu'])
            assert _inside(_store(y, mode), st, mode), (geo, family, mode, lanes)
        if family != 'constant':       # the bracket is no wider than a few units of the output's own rounding, or of 1e-3 of its scale
            assert float(st['bound'].max()) <= 2e-3 * max(1.0, float(np.abs(st['y']).max())), (geo, family, mode, float(st['bound'].max()))


def test_constant_groups_give_beta_plus_r_exactly():
    c = _case((2, 5, 7, 128, 8), 'constant', 'f32', normalised=False)
    y = R.emulate_f32(c['u'], c['gamma'], c['beta'], c['G'], R.EPS, c['S'], 4, c['resid'], None, True)
    want = np.maximum((c['beta'].astype(np.float32) + c['resid'].astype(np.float32)).astype(np.float32), 0).astype(np.float64)
    assert np.array_equal(y, want)


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_leaves_a_bracket(mistake):
    caught = []
    for family in ('real', 'offset'):
        for mode in MODES:
            for geo in ((2, 5, 7, 128, 8), CPU_RAGGED):
                c = _case(geo, family, mode)
                st = _statement(c)
                wrong = _statement(c, mistake=mistake)['y']
                if not _inside(_store(wrong, mode), st, mode):
                    caught.append((family, mode, geo))
    assert caught, mistake
    if mistake == 'sumsq':
        assert any(f == 'offset' and m == 'f32' for f, m, _ in caught), caught


# ------------------------------------------------------------------------------------------------ modules
def _expand(fixture, case):
    out = []
    for stage, first, count, t in case['runs']:
        sid, shapes = fixture['templates'][t]
        for i in range(first, first + count):
            out += [(('%s.%d.' % (stage, i) if stage else '') + suffix, tuple(shape)) for suffix, shape in zip(fixture['suffixes'][sid], shapes)]
    return out


def test_module_keys_and_shapes_equal_the_references():
    fixture = json.load(open(os.path.join(GOLDEN, 'gn_modules.json')))
    cases = fixture['cases']
    assert sorted(set(c['cls'] for c in cases)) == ['ResLayer', 'ResNet'] and len(cases) == 9
    for c in cases:
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c['kwargs'].items()}
        assert kw['norm_cfg'] == GN32
        mine = getattr(hvrnet_amd, c['cls'])(**kw).state_dict()
        theirs = _expand(fixture, c)
        assert len(theirs) > 25 and [(k, tuple(v.shape)) for k, v in mine.items()] == theirs, (c['cls'], kw)
        assert any(k.endswith('gn3.weight') for k, _ in theirs) and not any('bn' in k or 'running' in k for k, _ in theirs)


def golden_blocks():
    z = np.load(os.path.join(GOLDEN, 'g25_gn_block.npz'))
    cfg = dict(type='GN', num_groups=8)
    down = nn.Sequential(nn.Conv2d(128, 128, 1, stride=2, bias=False), nn.GroupNorm(8, 128))
    blocks = dict(a=backbone.Bottleneck(128, 32, stride=2, dilation=1, downsample=down, style='pytorch', norm_cfg=cfg),
                  b=backbone.Bottleneck(128, 32, stride=1, dilation=2, downsample=None, style='pytorch', norm_cfg=cfg))
    for name, blk in blocks.items():
        sd = {k[len(name) + 1:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith(name + '.') and k != name + '.out'}
        blk.load_state_dict(sd, strict=True)
    return z, blocks


def test_golden_blocks_load_strictly_and_say_what_they_are():
    z, blocks = golden_blocks()
    assert tuple(z['x'].shape) == (2, 128, 9, 11) and tuple(z['a.out'].shape) == (2, 128, 5, 6) and tuple(z['b.out'].shape) == (2, 128, 9, 11)
    a = blocks['a']
    assert isinstance(a.gn1, nn.GroupNorm) and isinstance(a.downsample[1], nn.GroupNorm) and a.gn1.num_groups == 8 and a.gn3.eps == 1e-5
    assert (a.gn_width, a.gn_width_groups) == (64, 16)       # 32 channels in 8 groups run as 64 in 16: eight groups of exact zeros behind them
    assert list(a.state_dict())[:3] == ['conv1.weight', 'gn1.weight', 'gn1.bias']
    # the f64 blocks are the statement's: conv -> GN -> ReLU chains in torch on the same parameters
    for name, blk in blocks.items():
        d = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + '.')}
        x = torch.from_numpy(z['x'])
        s, dil = (2, 1) if name == 'a' else (1, 2)
        h = F.relu(F.group_norm(F.conv2d(x, d['conv1.weight']), 8, d['gn1.weight'], d['gn1.bias'], 1e-5))
        h = F.relu(F.group_norm(F.conv2d(h, d['conv2.weight'], stride=s, padding=dil, dilation=dil), 8, d['gn2.weight'], d['gn2.bias'], 1e-5))
        y = F.group_norm(F.conv2d(h, d['conv3.weight']), 8, d['gn3.weight'], d['gn3.bias'], 1e-5)
        idn = x if name == 'b' else F.group_norm(F.conv2d(x, d['downsample.0.weight'], stride=2), 8, d['downsample.1.weight'], d['downsample.1.bias'], 1e-5)
        assert float((F.relu(y + idn) - d['out']).abs().max()) <= 1e-12


def _r50(**kw):
    base = dict(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), norm_cfg=GN32)
    base.update(kw)
    return hvrnet_amd.ResNet(**base)


def test_every_step_of_a_gn_net_is_gn():
    for style in ('pytorch', 'caffe'):
        net = _r50(style=style)
        for dtype in native.COMPUTE_DTYPES:
            for i in range(3):
                route = net.stage_route(i, 3, 32, 40, dtype)
                assert all(s.kind == 'gn' and not s.compact and not s.h1_in for s in route.steps) and not route.compact, (style, i, str(route))
                assert [s.downsample for s in route.steps] == [True] + [False] * (len(route.steps) - 1)
            assert not any(net._dead_pixels(i) for i in range(3))
    assert str(_r50().stage_route(1, 3, 32, 40, torch.bfloat16)) == 'downsample+gn, gn x3 -> 16x20'
    # a BatchNorm net beside it keeps its fused routes
    assert str(hvrnet_amd.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
               .stage_route(2, 3, 16, 20, torch.bfloat16)).count('gn') == 0


def test_synthetic_gn_checkpoint_loads_strictly():
    sd = synthetic.synth_state_dict(depth=50, norm='GN')
    net = _r50()
    head = hvrnet_amd.ResLayer(depth=50, stage=3, stride=1, dilation=2, external_conv=True, norm_cfg=GN32)
    net.load_state_dict({k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.')}, strict=True)
    head.load_state_dict({k[len('shared_head.'):]: v for k, v in sd.items() if k.startswith('shared_head.')}, strict=True)
    assert not any('running_mean' in k for k in sd if k.startswith(('backbone.', 'shared_head.')))
    g = sd['backbone.layer2.1.gn2.weight']
    assert 0.5 <= float(g.min()) and float(g.max()) <= 1.5 and abs(float(sd['backbone.layer2.1.gn2.bias'].std()) - 0.1) < 0.04
    # the default is untouched: the same keys and values as before the keyword existed
    a, b = synthetic.synth_state_dict(depth=50), synthetic.synth_state_dict(depth=50, norm='BN')
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and 'backbone.bn1.running_var' in a
    assert isinstance(head.layer4[0].gn1, nn.GroupNorm) and isinstance(head.layer4[0].downsample[1], nn.GroupNorm)
    assert not any(p.requires_grad for p in net.parameters())


def test_refusals_name_the_combination():
    kw = dict(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), norm_cfg=GN32)
    with pytest.raises(NotImplementedError, match='dcn together with GroupNorm'):
        hvrnet_amd.ResNet(dcn=dict(modulated=False, deformable_groups=1), stage_with_dcn=(False, True, True), **kw)
    with pytest.raises(NotImplementedError, match='gcb together with GroupNorm'):
        hvrnet_amd.ResNet(gcb=dict(ratio=1. / 16), stage_with_gcb=(False, True, True), **kw)
    with pytest.raises(NotImplementedError, match='gen_attention together with GroupNorm'):
        hvrnet_amd.ResNet(gen_attention=dict(spatial_range=-1, num_heads=8, attention_type='0010', kv_stride=2),
                          stage_with_gen_attention=((), (), (0,)), **kw)
    with pytest.raises(NotImplementedError, match='GroupNorm .* on ResNeXt with groups=32'):
        hvrnet_amd.ResNeXt(groups=32, base_width=4, **kw)
    with pytest.raises(NotImplementedError, match='GroupNorm .* on ResXLayer with groups=32'):
        hvrnet_amd.ResXLayer(depth=50, groups=32, base_width=4, norm_cfg=GN32)
    with pytest.raises(NotImplementedError, match='dcn together with GroupNorm'):
        hvrnet_amd.ResLayer(depth=50, norm_cfg=GN32, dcn=dict(modulated=False, deformable_groups=1))
    for name, arg in (('dcn', dict(modulated=False)), ('gcb', dict(ratio=0.25)), ('gen_attention', dict(num_heads=8))):
        with pytest.raises(NotImplementedError, match='%s on a Bottleneck under GroupNorm' % name):
            backbone.Bottleneck(256, 64, norm_cfg=GN32, **{name: arg})
    with pytest.raises(NotImplementedError, match='GroupNorm .* on a grouped Bottleneck'):
        backbone.Bottleneck(256, 64, norm_cfg=GN32, groups=32)
    for bad in ('SyncBN', 'LN'):
        with pytest.raises(NotImplementedError, match='norm_cfg type %r is not built' % bad):
            hvrnet_amd.ResNet(depth=50, norm_cfg=dict(type=bad))
    with pytest.raises((KeyError, AssertionError)):
        hvrnet_amd.ResNet(depth=50, norm_cfg=dict(type='GN'))
    for groups in (64, 3, 128):     # one channel per group on the stem; no divisor; more groups than the stem has channels
        with pytest.raises(NotImplementedError, match='num_groups=%d .* outside the kernels\' instance set' % groups):
            hvrnet_amd.ResNet(depth=50, norm_cfg=dict(type='GN', num_groups=groups))
    with pytest.raises(NotImplementedError, match='outside the kernels\' instance set'):
        backbone.Bottleneck(256, 64, norm_cfg=dict(type='GN', num_groups=64))     # conv1's 64 channels at one per group
    with pytest.raises(NotImplementedError, match='BatchNorm'):                   # Res2Net keeps refusing
        hvrnet_amd.Res2Net(norm_cfg=GN32)


def test_gn_models_are_inference_only():
    blk = backbone.Bottleneck(256, 64, norm_cfg=GN32)
    x = torch.zeros(1, 4, 4, 256)
    with pytest.raises(NotImplementedError, match='inference only: group normalisation has no backward'):
        blk.forward_train_nhwc(x)
    with pytest.raises(NotImplementedError, match='inference only: group normalisation has no backward'):
        _r50().forward_train_nhwc(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='inference only: group normalisation has no backward'):
        hvrnet_amd.ResLayer(depth=50, norm_cfg=GN32).forward_train_nhwc(torch.zeros(1, 4, 4, 1024))
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.group_norm(torch.zeros(1, 2, 2, 64), torch.ones(64), torch.zeros(64), 32, 1e-5)
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.group_norm_stats(torch.zeros(1, 2, 2, 64), 32)
    assert _r50().out_shape_nhwc(3, 128, 160) == hvrnet_amd.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1),
                                                                    out_indices=(2,)).out_shape_nhwc(3, 128, 160)
    assert _r50(frozen_stages=1, norm_eval=False).train().training is False


def test_detectors_refuse_to_train_a_gn_model():
    """HNMBRCNN.forward_train runs the backbone frozen, under no_grad, and would never reach the backbone's own refusal: the detectors'
    training entries refuse a GroupNorm backbone or shared head themselves, before anything runs."""
    from hvrnet_amd.config import hvr_config, selsa_config
    from hvrnet_amd.registry import build_detector
    for make in (hvr_config, selsa_config):
        for part in ('backbone', 'shared_head'):
            cfg = make(frame_interval=1, nms_post=16)
            cfg.model.backbone = dict(cfg.model.backbone, depth=50, **(dict(norm_cfg=GN32) if part == 'backbone' else {}))
            cfg.model.shared_head = dict(cfg.model.shared_head, depth=50, **(dict(norm_cfg=GN32) if part == 'shared_head' else {}))
            model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
            with pytest.raises(NotImplementedError, match='inference only: group normalisation has no backward'):
                model.forward_train(torch.zeros((9, 3, 64, 64)), [{}] * 9, [], [])
            if hasattr(model, 'forward_train_sampled'):
                with pytest.raises(NotImplementedError, match='inference only: group normalisation has no backward'):
                    model.forward_train_sampled(torch.zeros((3, 3, 64, 64)), None, None, None, None, None, None)
