"""CPU tests of the ResNeXt path: the f64 statement of the grouped 3x3 conv (tests/gconv_refs.py) against torch's grouped conv and
against its own mistakes, the reference's ResNeXt blocks (tests/golden/g21_resnext_block.npz) rebuilt from this project's Bottleneck,
the module contract (tests/golden/resnext_modules.json), the registry, the width arithmetic, the refusals, the routes of a grouped
stage and the shape query of hvr_conv3x3_grouped.  Nothing here needs a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import hvrnet_amd
from hvrnet_amd import backbone, native, registry
from tests import forward_kernel_refs as F
from tests import gconv_refs as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize('geom', G.GEOMETRIES, ids=lambda g: 'x'.join(str(v) for v in g))
def test_statement_equals_torch_grouped_conv(geom):
    B, H, W, C, Cg, s, d = geom
    c = G.real_case(geom, 'f32', seed=11)
    for relu in (False, True):
        ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], relu, s, d)
        want = torch.nn.functional.conv2d(c['x'].permute(0, 3, 1, 2), c['w'].permute(0, 3, 1, 2), c['bias'], stride=s, padding=d, dilation=d,
                                          groups=C // Cg).permute(0, 2, 3, 1)
        want = want.clamp(min=0.0) if relu else want
        assert tuple(ref.shape) == (B,) + G.out_hw(H, W, s) + (C,)
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all()) and bool((mag >= absxw).all())
    if C <= 128:
        sl = G.by_slices(c['x'], c['w'], c['bias'], True, s, d)
        assert float((ref - sl).abs().max()) <= 1e-12 * float(sl.abs().max())


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('Cg', G.CGS)
def test_every_mistake_leaves_the_bracket_on_real_operands(mode, Cg):
    geom = (2, 5, 7, 64, Cg, 2, 2)
    c = G.real_case(geom, mode, seed=23 + Cg)
    ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, 2, 2)
    lo, hi = G.gconv_bracket(ref, mag, absxw, Cg, mode)
    assert F.compare(F.round_stored(ref, mode), lo, hi, ref)[1] == 0          # the statement itself, stored, lies inside
    for mistake in G.MISTAKES:
        bad_ref = G.gconv_statement(c['x'], c['w'], c['bias'], True, 2, 2, mistake=mistake)[0]
        got = F.round_stored(bad_ref, mode)
        assert F.compare(got, lo, hi, ref)[1] > 0, (mistake, mode, Cg)


@pytest.mark.parametrize('mode', F.MODES)
def test_every_mistake_is_unequal_on_exact_operands(mode):
    for Cg in G.CGS:
        geom = (2, 5, 7, 64, Cg, 2, 2)
        for family in G.exact_families(mode):
            c = G.exact_gconv_case(geom, mode, seed=5 + Cg, family=family)
            ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, 2, 2)
            F.assert_exact(c['x'], c['w'], mag, c['q'], mode, ref)
            want = F.round_stored(ref, mode)
            for mistake in G.MISTAKES:
                got = F.round_stored(G.gconv_statement(c['x'], c['w'], c['bias'], True, 2, 2, mistake=mistake)[0], mode)
                assert int((got != want).sum()) > 0, (mistake, mode, Cg, family)


def test_geometry_bound_mistakes_are_noops_elsewhere():
    """'stride_phase' is a statement about stride 2 and 'dil1' about dilation 2: at stride 1 / dilation 1 they are the rule itself."""
    c = G.real_case((2, 5, 7, 64, 8, 1, 1), 'f32', seed=3)
    ref = G.gconv_statement(c['x'], c['w'], c['bias'], True, 1, 1)[0]
    for mistake in ('stride_phase', 'dil1'):
        assert torch.equal(ref, G.gconv_statement(c['x'], c['w'], c['bias'], True, 1, 1, mistake=mistake)[0])


# ------------------------------------------------------------------------------------------------ the reference's blocks
def _fold64(conv, bn):
    """(w [Cout, KH, KW, Cin / groups], bias) of conv + eval-mode BatchNorm in f64."""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return (conv.weight.detach() * scale[:, None, None, None]).permute(0, 2, 3, 1).contiguous(), bn.bias.detach() - bn.running_mean * scale


@pytest.mark.parametrize('name', ['a', 'b'])
def test_golden_resnext_blocks_from_this_projects_bottleneck(name):
    z = np.load(os.path.join(GOLDEN, 'g21_resnext_block.npz'))
    stride, dil = (2, 1) if name == 'a' else (1, 2)
    down = nn.Sequential(nn.Conv2d(128, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128)) if name == 'a' else None
    blk = backbone.Bottleneck(128, 32, stride, dil, down, style='pytorch', groups=8, base_width=16).double().eval()
    assert blk.width == 64 and tuple(blk.conv2.weight.shape) == (64, 8, 3, 3)
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + '.') and k != name + '.out'}
    blk.load_state_dict(sd, strict=True)
    p = dict(c1=_fold64(blk.conv1, blk.bn1), c2=_fold64(blk.conv2, blk.bn2), c3=_fold64(blk.conv3, blk.bn3))
    if down is not None:
        p['ds'] = _fold64(blk.downsample[0], blk.downsample[1])
    x = torch.from_numpy(z['x']).permute(0, 2, 3, 1)
    got = G.block_chain(x, p, stride, dil, 'pytorch', down is not None).permute(0, 3, 1, 2)
    want = torch.from_numpy(z[name + '.out'])
    assert got.shape == want.shape and float(want.abs().max()) > 1.0
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())


def _expand(fixture, case):
    """The ordered [(key, shape), ...] of a case from its runs [stage, first block, blocks, template]: a template is a list of key suffixes
    (by index) with their shapes, a key `stage.block.suffix` (the stem and a head's extra conv: the suffix alone)."""
    out = []
    for stage, first, count, t in case['runs']:
        sid, shapes = fixture['templates'][t]
        for i in range(first, first + count):
            out += [(('%s.%d.' % (stage, i) if stage else '') + suffix, tuple(shape)) for suffix, shape in zip(fixture['suffixes'][sid], shapes)]
    return out


def test_module_keys_and_shapes_equal_the_references():
    fixture = json.load(open(os.path.join(GOLDEN, 'resnext_modules.json')))
    cases = fixture['cases']
    assert sorted(set(c['cls'] for c in cases)) == ['ResNeXt', 'ResXLayer'] and len(cases) == 17
    for c in cases:
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c['kwargs'].items()}
        mine = getattr(hvrnet_amd, c['cls'])(**kw).state_dict()
        theirs = _expand(fixture, c)
        assert len(theirs) > 60 and [(k, tuple(v.shape)) for k, v in mine.items()] == theirs, (c['cls'], kw)


def test_registry_builds_resnext_and_resxlayer():
    net = registry.build_from_cfg(dict(type='ResNeXt', depth=50, groups=32, base_width=4, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1),
                                       out_indices=(2,), style='pytorch'), registry.BACKBONES)
    head = registry.build_from_cfg(dict(type='ResXLayer', depth=50, stage=3, stride=1, dilation=2, groups=32, base_width=4, external_conv=True),
                                   registry.SHARED_HEADS)
    assert isinstance(net, hvrnet_amd.ResNeXt) and isinstance(net, hvrnet_amd.ResNet) and isinstance(head, hvrnet_amd.ResXLayer)
    assert (net.groups, net.base_width, head.groups, head.base_width) == (32, 4, 32, 4)
    assert tuple(head.new_layer_1.conv.weight.shape) == (256, 2048, 1, 1)
    assert tuple(head.layer4[0].conv2.weight.shape) == (1024, 32, 3, 3) and head.layer4[0].conv2.dilation == (2, 2)
    assert not any(p.requires_grad for p in net.parameters())
    plain = hvrnet_amd.ResNeXt(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))      # groups = 1: a ResNet
    ref = hvrnet_amd.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert all(b.width == b.planes and b.groups == 1 for b in plain.modules() if isinstance(b, backbone.Bottleneck))


@pytest.mark.parametrize('groups,first', [(32, 128), (64, 256)])
def test_width_arithmetic_of_32x4d_and_64x4d(groups, first):
    net = hvrnet_amd.ResNeXt(depth=50, groups=groups, base_width=4)
    for i, name in enumerate(net.res_layers):
        for blk in getattr(net, name):
            assert blk.width == first * 2 ** i and blk.width // groups == 4 * 2 ** i and blk.planes == 64 * 2 ** i
            assert tuple(blk.conv1.weight.shape)[:2] == (blk.width, blk.inplanes)
            assert tuple(blk.conv2.weight.shape) == (blk.width, 4 * 2 ** i, 3, 3) and blk.conv2.groups == groups
            assert tuple(blk.conv3.weight.shape)[:2] == (4 * blk.planes, blk.width)
    assert net.feat_dim == 2048 and net.out_shape_nhwc(1, 64, 64) is None


def test_refusals():
    with pytest.raises(NotImplementedError, match='dcn'):
        backbone.Bottleneck(256, 64, groups=32, base_width=4, dcn=dict(modulated=False, deformable_groups=1, fallback_on_stride=False))
    with pytest.raises(NotImplementedError, match='dcn'):
        hvrnet_amd.ResNeXt(depth=50, groups=32, base_width=4, dcn=dict(modulated=False, deformable_groups=1, fallback_on_stride=False),
                           stage_with_dcn=(False, True, True, True))
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNeXt(depth=50, groups=32, gcb=dict(ratio=1. / 16))
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNeXt(depth=50, groups=32, conv_cfg=dict(type='ConvWS'))
    blk = backbone.Bottleneck(256, 64, groups=32, base_width=4)
    with pytest.raises(NotImplementedError, match='inference only'):
        blk.forward_train_nhwc(torch.zeros(1, 4, 4, 256))
    head = hvrnet_amd.ResXLayer(depth=50, stage=3, stride=1, dilation=2, groups=32, base_width=4, external_conv=True)
    with pytest.raises(NotImplementedError, match='inference only'):
        head.forward_train_nhwc(torch.zeros(1, 4, 4, 1024))
    with pytest.raises(NotImplementedError):        # CPU tensors, as everywhere
        head(torch.zeros(1, 1024, 4, 4))
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNeXt(depth=50, groups=32, base_width=4)(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        native.conv3x3_grouped(torch.zeros(1, 4, 4, 64), torch.zeros(64, 3, 3, 4), torch.zeros(64), True, 1, 1)
    with pytest.raises(TypeError):
        hvrnet_amd.ResLayer(depth=50, groups=32)


def test_a_grouped_stage_runs_at_full_resolution():
    """Dead-pixel compaction is not built for grouped stages: a caffe-style ResNeXt plans no 'close_sampled' / 'tail_next_live' step where
    the ResNet of the same shape does, and every close of a grouped block is one of 'conv', 'tail', 'tail_next'."""
    _lib()
    kw = dict(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
    plain, grouped = hvrnet_amd.ResNet(**kw), hvrnet_amd.ResNeXt(groups=32, base_width=4, **kw)
    for dt in (torch.bfloat16, torch.float16, native.SPLIT, torch.float32):
        H, W, compact = 152, 252, False
        for i in range(3):
            assert grouped._dead_pixels(i) is False
            blocks = list(getattr(grouped, grouped.res_layers[i]))
            assert grouped._live_store(i, blocks[-2], blocks[-1], 15, H, W, dt) is False
            r = grouped.stage_route(i, 15, H, W, dt, compact)
            assert not r.compact and all(s.kind in ('conv', 'tail', 'tail_next') and not s.compact for s in r.steps), str(r)
            assert r.out_hw == ((H - 1) // kw['strides'][i] + 1, (W - 1) // kw['strides'][i] + 1)
            (H, W), compact = r.out_hw, r.compact
    assert plain._dead_pixels(0) and plain.stage_route(0, 15, 152, 252, torch.bfloat16).compact


# ------------------------------------------------------------------------------------------------ the shape query
def test_grouped_conv_shape_query():
    lib = _lib()
    ok = native.conv3x3_grouped_supported
    for dt in (torch.bfloat16, torch.float16):
        # every stage of X-101 32x4d and 64x4d on a 15-frame window, res5 at dilation 2, and the stride-2 first blocks
        for groups in (32, 64):
            for i, (H, W) in enumerate([(152, 252), (76, 126), (38, 63), (38, 63)]):
                C = groups * 4 * 2 ** i
                assert ok(15, H, W, C, groups, 1, 2 if i == 3 else 1, dt), (groups, i)
            assert ok(15, 152, 252, groups * 8, groups, 2, 1, dt) and ok(15, 76, 126, groups * 16, groups, 2, 1, dt)
        for B, H, W, C, Cg, s, d in G.GEOMETRIES:
            assert ok(B, H, W, C, C // Cg, s, d, dt)
        assert not ok(2, 5, 7, 64, 32, 1, 1, dt)            # Cg = 2
        assert not ok(2, 5, 7, 128, 2, 1, 1, dt)            # Cg = 64
        assert not ok(2, 5, 7, 192, 16, 1, 1, dt)           # Cg = 12
        assert not ok(2, 5, 7, 96, 3, 1, 1, dt)             # C % 64 != 0
        assert not ok(2, 5, 7, 32, 8, 1, 1, dt)             # C < 64
        assert not ok(1, 4, 4, 4096, 128, 1, 1, dt)         # C > 2048
        assert not ok(2, 5, 7, 64, 5, 1, 1, dt)             # groups does not divide C
        assert not ok(2, 5, 7, 64, 8, 3, 1, dt)             # stride 3
        assert not ok(2, 5, 7, 64, 8, 1, 3, dt)             # dilation 3
        assert not ok(2, 5, 7, 64, 8, 1, 1, dt, pad=2) and not ok(2, 5, 7, 64, 8, 1, 2, dt, pad=1) and not ok(2, 5, 7, 64, 8, 1, 1, dt, pad=0)
        assert not ok(0, 5, 7, 64, 8, 1, 1, dt)
    for dt in (torch.float32, native.SPLIT):                # these modes run the dense route
        assert not ok(15, 38, 63, 512, 32, 1, 1, dt)
    # pointers are inspected for alignment only; the launching entry refuses the same descriptors with a message, before any launch
    d = native.GConvDesc(x=1 << 20, w=1 << 20, y=1 << 20, bias=1 << 20, B=2, H=5, W=7, C=64, groups=8, stride=1, pad=1, dil=1, relu=1,
                         dtype=native.HVR_BF16)
    assert lib.hvr_conv3x3_grouped_supported(ctypes.byref(d)) == 1
    d.x = (1 << 20) + 8
    assert lib.hvr_conv3x3_grouped_supported(ctypes.byref(d)) == 0
    d.x, d.bias = 1 << 20, None
    assert lib.hvr_conv3x3_grouped_supported(ctypes.byref(d)) == 0
    d.bias, d.pad = 1 << 20, 2
    assert lib.hvr_conv3x3_grouped(ctypes.byref(d), None) == -1 and b'pad' in lib.hvr_last_error()
    d.pad, d.dtype = 1, native.HVR_F32
    assert lib.hvr_conv3x3_grouped(ctypes.byref(d), None) == -2 and b'dense' in lib.hvr_last_error()
    assert lib.hvr_abi_version() == 7
