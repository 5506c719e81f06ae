"""CPU tests of the Res2Net path: the f64 statements of tests/res2_refs.py against torch.nn.functional and the reference's own blocks
(tests/golden/g22_res2net_block.npz), the padded-slice layout, the stated mistakes, module keys against the reference's
(tests/golden/res2net_modules.json), the registry, the width arithmetic, the refusals and the shape query of hvr_res2_conv3x3 (which
builds the library; no GPU is needed)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import hvrnet_amd
from hvrnet_amd import backbone, native, registry, synthetic
from tests import forward_kernel_refs as F
from tests import res2_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _golden():
    return np.load(os.path.join(GOLDEN, 'g22_res2net_block.npz'))


def _sd(z, name):
    return {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + '.') and k.split('.')[-1] not in ('x', 'out', 'out_f32')}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


BLOCKS = dict(a=dict(stype='stage', stride=2, dil=1, downsample=True), b=dict(stype='normal', stride=1, dil=2, downsample=False))


def _block_ref(z, name, mistake=None, padded=False, stride=None):
    kw = dict(BLOCKS[name], **({} if stride is None else dict(stride=stride)))
    p = R.fold_block(_sd(z, name), 3, kw['downsample'])
    width = 13
    if padded:
        p, width = R.pad_layout(p, 13, 4, mistake), R.pad_width(13)
    y = R.block_statement(_nhwc(torch.from_numpy(z[name + '.x'])), p, width, 4, kw['stype'], kw['stride'], kw['dil'], mistake)
    return y.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ statements
@pytest.mark.parametrize('geom', [g for g in R.SMALL if g[3] in (13, 52)], ids=lambda g: 'x'.join(str(v) for v in g))
def test_slice_conv_statement_equals_torch(geom):
    """The slice conv with and without the pre-add against torch.nn.functional.conv2d on the slices, 1e-10; the other slices hold NaN."""
    B, H, W, width, s, d = geom
    Wp = R.pad_width(width)
    for with_add in (False, True):
        c = R.real_slice_case(geom, 'f32', 31, with_add)
        x = torch.full((B, H, W, 4 * Wp), float('nan'), dtype=torch.float64)
        x[..., 2 * Wp:3 * Wp] = c['x']
        a = None
        if with_add:
            a = torch.full((B, H, W, 3 * Wp), float('nan'), dtype=torch.float64)
            a[..., :Wp] = c['add']
        ref, mag, absxw = R.slice_conv_statement(x, 2 * Wp, c['w'], c['bias'], a, 0, True, s, d, 'f32')
        sp = c['x'] if not with_add else (c['x'] + c['add']).float().double()
        want = TF.conv2d(sp.permute(0, 3, 1, 2), c['w'].permute(0, 3, 1, 2), c['bias'], stride=s, padding=d, dilation=d).clamp(min=0).permute(0, 2, 3, 1)
        assert bool(torch.isfinite(ref).all()) and float((ref - want).abs().max()) <= 1e-10
        assert bool((ref[..., width:] == 0).all()), 'the pad channels of the output are exact zeros'
        assert bool((mag >= ref.abs() - 1e-12).all()) and bool((absxw <= mag + 1e-12).all())


def test_operand_is_the_rounded_f32_sum():
    g = torch.Generator().manual_seed(3)
    for mode, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
        x, a = torch.randn((4096,), generator=g).to(dt), (torch.randn((4096,), generator=g) * 3).to(dt)
        assert torch.equal(R.operand(x, a, mode), (x.float() + a.float()).to(dt).double())
    x, a = torch.randn((4096,), generator=g), torch.randn((4096,), generator=g)
    assert torch.equal(R.operand(x, a, 'f32'), (x + a).double())
    assert torch.equal(R.operand(x, None, 'f32'), x.double())


POOLS = [(3, 1, 1, False, True), (3, 2, 1, False, True), (2, 2, 0, True, False), (1, 1, 0, False, True)]


@pytest.mark.parametrize('hw', [(9, 11), (10, 12)])
@pytest.mark.parametrize('pool', POOLS)
def test_pool_statement_equals_torch(hw, pool):
    """The three uses (the 'stage' pool at both strides, the shortcut pool, the copy) against torch.nn.functional.avg_pool2d, 1e-10."""
    k, s, p, ce, inc = pool
    x = torch.randn((2,) + hw + (8,), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    ref, mabs, taps = R.pool_statement(x, k, s, p, ce, inc)
    want = TF.avg_pool2d(x.permute(0, 3, 1, 2), k, s, p, ceil_mode=ce, count_include_pad=inc).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == tuple(want.shape) == (2,) + native.avgpool_out_hw(hw[0], hw[1], k, s, p, ce) + (8,)
    assert float((ref - want).abs().max()) <= 1e-10 and taps == k * k and bool((mabs >= ref.abs() - 1e-12).all())
    if k == 1:
        assert torch.equal(ref, x)


def test_ceil_mode_has_edge_windows_of_two_and_one_elements():
    x = torch.ones((1, 9, 11, 1), dtype=torch.float64)
    x[0, 8, :, 0], x[0, :, 10, 0], x[0, 8, 10, 0] = 2.0, 3.0, 7.0
    ref = R.pool_statement(x, 2, 2, 0, True, False)[0]
    assert tuple(ref.shape) == (1, 5, 6, 1) and float(ref[0, 4, 5, 0]) == 7.0 and float(ref[0, 4, 0, 0]) == 2.0 and float(ref[0, 0, 5, 0]) == 3.0


def test_stem_first_statement_equals_torch():
    g = torch.Generator().manual_seed(4)
    img, w, b = torch.randn((2, 3, 33, 41), generator=g, dtype=torch.float64), torch.randn((32, 3, 3, 3), generator=g, dtype=torch.float64), \
        torch.randn((32,), generator=g, dtype=torch.float64)
    ref, mag = R.stem_first_statement(img, w, b)
    want = TF.conv2d(img, w.permute(0, 3, 1, 2), b, stride=2, padding=1).clamp(min=0).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (2, 17, 21, 32) and float((ref - want).abs().max()) <= 1e-10


@pytest.mark.parametrize('name', ['a', 'b'])
def test_block_statement_equals_the_references_block(name):
    """The chain of statements over folded weights equals the reference's own f64 evaluation of its Bottle2neck, in the real layout and
    in the padded-slice layout (zero weights add exact zeros), to 1e-10; the reference's own f32 run lies inside the f32 bound that the
    GPU test holds this project's f32 mode to, so that bound is never tighter than the reference's own f32 arithmetic."""
    z = _golden()
    want = torch.from_numpy(z[name + '.out'])
    for padded in (False, True):
        y = _block_ref(z, name, padded=padded)
        assert tuple(y.shape) == tuple(want.shape) and float((y - want).abs().max()) <= 1e-10, (name, padded)
    f32 = torch.from_numpy(z[name + '.out_f32']).double()
    assert float((f32 - want).abs().max()) <= R.block_bound_f32(float(want.abs().max()))


def test_stem_chain_equals_the_references_stem():
    z = _golden()
    sd = _sd(z, 'stem')
    x = _nhwc(torch.from_numpy(z['stem.x']))
    y = R.stem_first_statement(x.permute(0, 3, 1, 2), *R.fold(sd, 'conv1.0', 'conv1.1'))[0]
    y = F.conv_statement(y, *R.fold(sd, 'conv1.3', 'conv1.4'), None, True, 1, 1, 1)[0]
    y = F.conv_statement(y, *R.fold(sd, 'conv1.6', 'bn1'), None, True, 1, 1, 1)[0]
    y = F.maxpool_statement(y)
    want = _nhwc(torch.from_numpy(z['stem.out']))
    assert tuple(y.shape) == tuple(want.shape) == (1, 9, 11, 64) and float((y - want).abs().max()) <= 1e-10 * float(want.abs().max())
    f32 = _nhwc(torch.from_numpy(z['stem.out_f32'])).double()
    assert float((f32 - want).abs().max()) <= R.stem_bound_f32(float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ the stated mistakes
# mistake -> the golden block it shows on ('first_dilated': block a is the 'stage' block that must stay at dilation 1)
MISTAKE_BLOCK = dict(add_same_slice='b', add_in_stage='a', pool_in_normal='b', pool_valid_count='a', shortcut_floor='a', first_dilated='a',
                     pad_nonzero='b')


def _exact_block(name, mistake=None, padded=False, stride=None):
    """The golden block's structure on exact operands: integer inputs, integer weights of at most two bits, no BatchNorm shift."""
    kw = dict(BLOCKS[name], **({} if stride is None else dict(stride=stride)))
    g = torch.Generator().manual_seed(17)
    cin = 64 if name == 'a' else 128
    ints = lambda shape, top: torch.randint(-top, top + 1, shape, generator=g).double()
    p = dict(c1=(ints((52, 1, 1, cin), 2), ints((52,), 3)), br=[(ints((13, 3, 3, 13), 2), ints((13,), 3)) for _ in range(3)],
             c3=(ints((128, 1, 1, 52), 2), ints((128,), 3)))
    if kw['downsample']:
        p['ds'] = (ints((128, 1, 1, cin), 2) * 36.0, ints((128,), 3))     # (x 36: the shortcut pool's divisors 1, 2 and 4 leave integers)
    x = ints((2, 9, 11, cin), 3) * (4.0 if name == 'a' else 1.0)
    width = 13
    if padded:
        p, width = R.pad_layout(p, 13, 4, mistake), 32
    return R.block_statement(x, p, width, 4, kw['stype'], kw['stride'], kw['dil'], mistake)


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_stated_mistake_is_caught(mistake):
    """On the golden blocks (real operands) each mistake leaves the f32 bound of the block by a wide margin; on exact operands (integers:
    every value of the chain is an integer or, behind the 'stage' pool, a multiple of 1/9 evaluated alike) it is unequal.
    'add_in_stage' is shown on block a run at stride 1 (the sum of a stride-2 branch output and a full-resolution slice does not exist),
    against the statement of that block without the mistake."""
    z = _golden()
    name = MISTAKE_BLOCK[mistake]
    padded = mistake == 'pad_nonzero'
    stride = 1 if mistake == 'add_in_stage' else None
    want = torch.from_numpy(z[name + '.out']) if stride is None else _block_ref(z, name, stride=stride)
    wrong = _block_ref(z, name, mistake, padded=padded, stride=stride)
    err = float((wrong - want).abs().max())
    assert err > 20 * R.block_bound_f32(float(want.abs().max())), (mistake, err)
    right, off = _exact_block(name, None, padded, stride), _exact_block(name, mistake, padded, stride)
    assert torch.equal(right, _exact_block(name, stride=stride)) and not torch.equal(right, off), mistake


def test_pool_mistakes_at_the_pool():
    x = torch.randn((1, 9, 11, 4), generator=torch.Generator().manual_seed(2), dtype=torch.float64).abs() + 0.5
    ref, mabs, taps = R.pool_statement(x, 3, 2, 1, False, True)
    lo, hi = R.pool_bracket(ref, mabs, taps, 'f32')
    assert F.compare(R.pool_statement(x, 3, 2, 1, False, True, 'pool_valid_count')[0], lo, hi, ref)[1] > 0
    ref, mabs, taps = R.pool_statement(x, 2, 2, 0, True, False)
    lo, hi = R.pool_bracket(ref, mabs, taps, 'f32')
    assert F.compare(R.pool_statement(x, 2, 2, 0, True, False, 'shortcut_floor')[0], lo, hi, ref)[1] > 0
    assert F.compare(ref, lo, hi, ref)[1] == 0


# ------------------------------------------------------------------------------------------------ modules, registry, widths
def _expand(fixture, case):
    """tests/test_gconv_refs.py: _expand (the run-length form of resnext_modules.json)."""
    out = []
    for stage, first, count, t in case['runs']:
        sid, shapes = fixture['templates'][t]
        for i in range(first, first + count):
            out += [(('%s.%d.' % (stage, i) if stage else '') + suffix, tuple(shape)) for suffix, shape in zip(fixture['suffixes'][sid], shapes)]
    return out


def test_module_keys_and_shapes_equal_the_references():
    fixture = json.load(open(os.path.join(GOLDEN, 'res2net_modules.json')))
    cases = fixture['cases']
    assert [c['cls'] for c in cases] == ['Res2Net', 'Res2Net', 'Res2Layer']
    for c in cases:
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c['kwargs'].items()}
        mine = getattr(hvrnet_amd, c['cls'])(**kw).state_dict()
        theirs = _expand(fixture, c)
        assert len(theirs) > 90 and [(k, tuple(v.shape)) for k, v in mine.items()] == theirs, (c['cls'], kw)
    assert len(_expand(fixture, cases[0])) == len(_expand(fixture, cases[1])) == 936      # three stages whatever num_stages says


def test_registry_builds_res2net_and_res2layer():
    net = registry.build_from_cfg(dict(type='Res2Net', num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='pytorch'),
                                  registry.BACKBONES)
    head = registry.build_from_cfg(dict(type='Res2Layer', depth=101, stage=3, stride=1, dilation=2, external_conv=True), registry.SHARED_HEADS)
    assert isinstance(net, hvrnet_amd.Res2Net) and isinstance(head, hvrnet_amd.Res2Layer)
    assert [len(getattr(net, n)) for n in net.res_layers] == [3, 4, 23] and net.out_shape_nhwc(2, 65, 97) == (2, 5, 7, 1024)
    assert tuple(head.new_layer_1.conv.weight.shape) == (256, 2048, 1, 1)
    blocks = list(head.layer4)
    assert [(b.stype, b.stride, b.dilation) for b in blocks] == [('stage', 1, 1), ('normal', 1, 2), ('normal', 1, 2)]
    assert blocks[0].pool.kernel_size == 3 and blocks[0].pool.stride == 1 and blocks[0].downsample[0].kernel_size == 1
    assert [k for k in blocks[0].state_dict() if k.startswith('downsample')][0] == 'downsample.1.weight'
    assert not any(p.requires_grad for p in net.parameters())
    # the synthetic checkpoint loads strictly, in the reference's key order
    sd = synthetic.synth_state_dict(arch='res2net')
    for mod, prefix in ((net, 'backbone.'), (head, 'shared_head.')):
        sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        assert list(sub) == list(mod.state_dict())
        mod.load_state_dict(sub, strict=True)
    assert list(synthetic.synth_state_dict()) == list(synthetic.synth_state_dict(arch='resnet')) and 'backbone.conv1.weight' in synthetic.synth_state_dict()


def test_width_arithmetic():
    net = hvrnet_amd.Res2Net(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    head = hvrnet_amd.Res2Layer(101)
    got = [(getattr(net, n)[0].width, getattr(net, n)[0].wp) for n in net.res_layers] + [(head.layer4[0].width, head.layer4[0].wp)]
    assert got == [(26, 32), (52, 64), (104, 128), (208, 224)] == list(R.WIDTHS.items())
    assert all(native.res2_pad_width(w) == wp == R.pad_width(w) for w, wp in R.WIDTHS.items()) and native.RES2_WIDTHS == tuple(R.WIDTHS.values())
    assert backbone.Bottle2neck(64, 32).width == 13 and backbone.Bottle2neck(64, 32).wp == 32


def test_packed_weights_keep_the_pad_channels_at_zero():
    """Bottle2neck._pack in f32 on the CPU (no kernel runs): the packed tensors are pad_layout's of the folded weights."""
    z = _golden()
    blk = backbone.make_res2_layer(backbone.Bottle2neck, 64, 32, 1, 26, 4, stride=2)[0]
    blk.load_state_dict({k: v.float() for k, v in _sd(z, 'a').items()}, strict=True)
    p = blk._pack(torch.float32)
    q = R.pad_layout(R.fold_block(_sd(z, 'a'), 3, True), 13, 4)
    assert tuple(p['c1'][0].shape) == (128, 1, 1, 64) and tuple(p['c3'][0].shape) == (128, 1, 1, 128)
    for mine, theirs in [(p['c1'], q['c1']), (p['c3'], q['c3']), (p['ds'], q['ds'])] + [((w.w32, b), t) for (w, b), t in zip(p['br'], q['br'])]:
        for m, t in zip(mine, theirs):
            assert tuple(m.shape) == tuple(t.shape) and float((m.double() - t).abs().max()) <= 1e-6 and bool(((t == 0) <= (m == 0)).all())
    assert p['br'][0][0].dense().shape[3] == 32 and native.Res2Weight(p['br'][0][0].w32, torch.bfloat16).dense().shape[3] == 64


# ------------------------------------------------------------------------------------------------ refusals and the shape query
def test_refusals():
    ok = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    with pytest.raises(NotImplementedError, match='scale == 1'):
        backbone.Bottle2neck(64, 32, scale=1)
    for kw in (dict(dcn=dict(modulated=False)), dict(gcb=dict(ratio=0.25)), dict(gen_attention=dict()), dict(conv_cfg=dict(type='ConvWS'))):
        with pytest.raises(NotImplementedError, match='dcn / gcb / gen_attention / conv_cfg'):
            hvrnet_amd.Res2Net(**dict(ok, **kw))
    with pytest.raises(NotImplementedError, match='BatchNorm'):
        hvrnet_amd.Res2Net(**dict(ok, norm_cfg=dict(type='GN', num_groups=32)))
    with pytest.raises(NotImplementedError, match='BatchNorm'):
        hvrnet_amd.Res2Layer(101, norm_cfg=dict(type='GN', num_groups=32))
    with pytest.raises(NotImplementedError, match='dcn'):
        hvrnet_amd.Res2Layer(101, dcn=dict(modulated=False))
    with pytest.raises(ValueError, match='strides'):
        hvrnet_amd.Res2Net(**dict(ok, strides=(1, 2, 1)))
    with pytest.raises(ValueError, match='dilation'):
        hvrnet_amd.Res2Net(**dict(ok, dilations=(1, 1, 2)))
    with pytest.raises(KeyError):
        hvrnet_amd.Res2Layer(50)
    net, head = hvrnet_amd.Res2Net(**ok), hvrnet_amd.Res2Layer(101, stride=1, dilation=2, external_conv=True)
    for mod in (net, head):
        with pytest.raises(NotImplementedError, match='load_state_dict'):
            mod.init_weights(pretrained='res2net101_v1b_26w_4s.pth')
    with pytest.raises(NotImplementedError, match='GPU only'):
        net(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(NotImplementedError, match='GPU only'):
        head(torch.zeros((1, 1024, 4, 4)))
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.res2_conv3x3(torch.zeros((1, 4, 4, 32)), 0, torch.zeros((32, 3, 3, 32)), torch.zeros((32,)))
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.avgpool_nhwc(torch.zeros((1, 4, 4, 32)), 3, 1, 1)
    for mod in (net, head, net.layer1[0]):
        with pytest.raises(NotImplementedError, match='inference only'):
            mod.forward_train_nhwc(torch.zeros((1, 4, 4, 64)))


def test_supported_by_shape():
    """hvr_res2_conv3x3_supported: the instance set of include/hvr_hip.h, nothing launched (placeholder addresses)."""
    q = native.res2_conv3x3_supported
    for Wp in native.RES2_WIDTHS:
        for dt in (torch.bfloat16, torch.float16):
            assert all(q(15, 38, 63, Wp, s, d, dt) and q(15, 38, 63, Wp, s, d, dt, add=True, add_off=Wp) for s in (1, 2) for d in (1, 2))
        assert not q(15, 38, 63, Wp, dtype=torch.float32) and not q(15, 38, 63, Wp, dtype=native.SPLIT)
    for Wp in (16, 96, 160, 192, 256):
        assert not q(2, 5, 7, Wp)
    assert not q(2, 5, 7, 64, stride=3) and not q(2, 5, 7, 64, dil=3) and not q(2, 5, 7, 64, dil=1, pad=2) and not q(0, 5, 7, 64)
    assert not q(2, 5, 7, 64, x_off=16) and not q(2, 5, 7, 64, ldx=200) and not q(2, 5, 7, 64, x_off=224) and not q(2, 5, 7, 64, y_off=48)
    assert q(2, 5, 7, 64, ldx=64, ldy=64) and q(2, 5, 7, 64, ldx=512, x_off=448)
    assert not q(1 << 15, 512, 512, 32, ldx=32, ldy=32)      # 2^33 output pixels
    # the automatic route: the kernel where tools/res2_bench.py measured it ahead, the composite form elsewhere
    assert native.RES2_KERNEL_WIDTHS[torch.bfloat16] == native.RES2_KERNEL_WIDTHS[torch.float16] and torch.float32 not in native.RES2_KERNEL_WIDTHS
