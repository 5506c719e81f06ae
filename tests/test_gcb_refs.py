"""CPU tests of the global context block's statements (tests/gcb_refs.py), its fixtures made by running the reference
(tests/golden/make_gcb_golden.py) and the module surface: registry, keys, strict loading, assertions, initialisation, routes, refusals."""
import json
import os

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import backbone, ops, synthetic as S
from hvrnet_amd.registry import BACKBONES, build_from_cfg
from tests import gcb_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GCB = dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))


# ------------------------------------------------------------------------------------------------ the statement and its mistakes
def _case(seed=5, shape=(3, 9, 11, 128), R_=16, w1_scale=1.0):
    return R.real_case(shape, 'f32', seed, 'att', ('channel_add', 'channel_mul'), R_, True, w1_scale)


def test_statement_is_the_torch_formula():
    """The statement against torch's own ops in f64 (softmax, layer_norm, sigmoid) on the context block's formula."""
    c = _case()
    u, prm = torch.from_numpy(c['u']), c['prm']
    a = torch.softmax(u @ torch.from_numpy(prm['wm']), 1)
    ctx = torch.einsum('bp,bpc->bc', a, u)

    def branch(br):
        w1, b1, g, be, w2, b2 = [torch.from_numpy(t) for t in br]
        h = torch.nn.functional.layer_norm(ctx @ w1.T + b1, (w1.shape[0],), g, be, 1e-5)
        return torch.relu(h) @ w2.T + b2
    y = torch.relu(u * torch.sigmoid(branch(prm['mul']))[:, None] + branch(prm['add'])[:, None] + torch.from_numpy(c['resid']))
    got = R.context_statement(c['u'], prm, c['resid'], True)['y']
    assert np.abs(got - y.numpy()).max() < 1e-12 and np.abs(got).max() > 1


def test_mask_bias_is_invariant():
    """conv_mask.bias shifts every logit of a frame alike: the weights are the same to f64 noise, so the kernels need not take it."""
    c = _case()
    a0 = R.pool_statement(c['u'], c['prm']['wm'], 0.0)
    for bm in (0.37, -55.0, 1e3):
        a1 = R.pool_statement(c['u'], c['prm']['wm'], bm)
        assert np.abs(a1['l'] - a0['l'] - bm).max() < 1e-9 and np.abs(a1['ctx'] - a0['ctx']).max() < 1e-12


def test_every_step_mistake_lands_outside_its_bound():
    """Each named mistake of the three steps, at the link where it is made, against that link's f32 bound on these inputs."""
    c = _case()
    u, prm = c['u'], c['prm']
    r = R.context_statement(u, prm, c['resid'], True)
    dctx = R.pool_bound(u, prm['wm'], r)
    assert (dctx / np.abs(r['ctx']).max()).max() < 1e-2
    for mk in ('softmax_channels', 'softmax_batch'):
        assert R.outside(R.pool_statement(u, prm['wm'], 0.0, mk)['ctx'], r['ctx'], dctx) > 0, mk
    # (the transform on a context it is handed exactly: its own roundings only, as the GPU tests hold it on the device's context)
    dm, dt = R.transform_bound(r['ctx'], np.zeros_like(dctx), prm['mul'], prm['add'])
    assert dm.max() < 1e-2 and dt.max() < 1e-2
    m, t = R.transform_statement(r['ctx'], prm['mul'], prm['add'], 'ln_unbiased')
    assert R.outside(m, r['m'], dm) > 0 and R.outside(t, r['t'], dt) > 0
    m, t = R.transform_statement(r['ctx'], prm['mul'], prm['add'], 'no_sigmoid')
    assert R.outside(m, r['m'], dm) > 0
    # eps outside the root shows where the variance is small: the same block with W1 and b1 a hundredth as large
    cs = _case(w1_scale=1e-2)
    rs = R.context_statement(cs['u'], cs['prm'], cs['resid'], True)
    dms, dts = R.transform_bound(rs['ctx'], np.zeros_like(dctx), cs['prm']['mul'], cs['prm']['add'])
    m, t = R.transform_statement(rs['ctx'], cs['prm']['mul'], cs['prm']['add'], 'ln_eps_outside')
    assert R.outside(m, rs['m'], dms) > 0 and R.outside(t, rs['t'], dts) > 0
    for mode in R.MODES:
        b = R.apply_bound(u, r['m'], r['t'], c['resid'], None, None, mode, r['y'])
        for mk in ('add_before_mul', 'relu_inside'):
            assert R.outside(R.apply_statement(u, r['m'], r['t'], c['resid'], True, mk), r['y'], b) > 0, (mk, mode)
        assert R.outside(r['y'], r['y'], b) == 0
    # the chained bound holds the statement itself and nothing is hidden by NaN
    assert np.isfinite(R.context_bound(u, prm, c['resid'], 'f32', r)).all()


def test_overflow_family_needs_the_running_maximum():
    for peak in ('first', 'last'):
        c = R.overflow_case(R.SHAPES[2], 'f32', 77, peak)
        r = R.context_statement(c['u'], c['prm'], c['resid'], True)
        with np.errstate(over='ignore'):
            assert np.isinf(np.exp(np.float32(r['l'].max())))
        S_, chunk = R.splits(3, 37 * 53)
        top = r['l'].argmax(1) // chunk
        assert (top == (0 if peak == 'first' else S_ - 1)).all()
        assert float(np.exp(np.float32(r['l'][:, c['lo']].max() - r['l'].max()))) == 0.0
        bad = R.context_statement(c['u'], c['prm'], c['resid'], True, 'no_max')
        assert not np.isfinite(bad['ctx']).all()
        assert R.outside(bad['ctx'], r['ctx'], R.pool_bound(c['u'], c['prm']['wm'], r)) > 0
        assert np.isfinite(r['y']).all() and (R.pool_bound(c['u'], c['prm']['wm'], r) / np.abs(r['ctx']).max()).max() < 1e-2


def test_splits_are_a_function_of_the_shape():
    assert R.splits(1, 1) == (1, 1) and R.splits(2, 63) == (1, 63) and R.splits(3, 1961) == (31, 64) and R.splits(15, 9576)[0] == 68
    for B, P in ((1, 1), (1, 64), (1, 65), (7, 300), (15, 2394), (2000, 50), (1, 10 ** 6)):
        S_, chunk = R.splits(B, P)
        assert 1 <= S_ <= 256 and (S_ - 1) * chunk < P <= S_ * chunk


def test_planes_truncate():
    assert R.planes_of(256, 0.3) == 76 and R.planes_of(256, 0.3, 'round_planes') == 77
    cb = ops.ContextBlock(256, 0.3)
    assert cb.planes == 76 and tuple(cb.channel_add_conv[0].weight.shape) == (76, 256, 1, 1)
    wrong = {k: (torch.zeros((77, 256, 1, 1)) if k == 'channel_add_conv.0.weight' else v) for k, v in cb.state_dict().items()}
    with pytest.raises(RuntimeError):
        cb.load_state_dict(wrong, strict=True)     # a round() build would hold 77 rows: such a checkpoint does not load


# ------------------------------------------------------------------------------------------------ fixtures made by running the reference
def _sd(z, name):
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '.') and k.split('.')[-1] not in ('x', 'out', 'out_f32')}


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _golden(name):
    z = np.load(os.path.join(GOLDEN, 'g23_gcb_block.npz'))
    return _sd(z, name), _nhwc(z[name + '.x']), _nhwc(z[name + '.out']), _nhwc(z[name + '.out_f32'])


def test_fixture_is_small_and_float32_valued():
    path = os.path.join(GOLDEN, 'g23_gcb_block.npz')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, 'g21_resnext_block.npz'))
    z = np.load(path)
    for k in z.files:
        if z[k].dtype == np.float64 and not k.endswith('.out'):
            assert np.array_equal(z[k], z[k].astype(np.float32).astype(np.float64)), k
    for name in ('ca', 'pa', 'pb'):     # the last convs carry values: the blocks are not the identity
        assert all(np.abs(z[k]).max() > 0 for k in z.files if k.startswith(name + '.') and k.endswith('_conv.3.weight'))


@pytest.mark.parametrize('name', ('ca', 'cb'))
def test_statement_reproduces_the_stand_alone_blocks(name):
    sd, x, out, out32 = _golden(name)
    B, H, W, C = x.shape
    prm = R.block_params(sd, '')
    assert (prm.get('wm') is None) == (name == 'cb') and (prm['add'] is None) == (name == 'cb')
    u = x.reshape(B, H * W, C)
    r = R.context_statement(u, prm)
    assert np.abs(r['y'].reshape(out.shape) - out).max() < 1e-12 * np.abs(out).max()
    assert R.outside(out32.reshape(u.shape).astype(np.float64), r['y'], R.context_bound(u, prm, None, 'f32', r)) == 0
    assert np.abs(out32 - out).max() <= R.block_bound_f32(np.abs(out).max())


@pytest.mark.parametrize('name,stride', (('pa', 2), ('pb', 1)))
def test_statement_reproduces_the_bottlenecks(name, stride):
    sd, x, out, out32 = _golden(name)
    y = R.bottleneck_statement(x, sd, stride=stride)
    assert y.shape == out.shape and np.abs(y - out).max() < 1e-11 * np.abs(out).max()
    bound = R.block_bound_f32(np.abs(out).max())
    assert np.abs(out32 - out).max() <= bound
    # (the LayerNorm mistakes move the output by less than the block's f32 bound here -- R = 32 and 8 rows, a variance of order one --:
    # they are shown at the step, test_every_step_mistake_lands_outside_its_bound)
    mistakes = ['after_residual', 'before_bn3', 'relu_inside', 'softmax_channels', 'softmax_batch']
    mistakes += ['add_before_mul', 'no_sigmoid'] if name == 'pa' else []
    if name == 'pb':
        mistakes.remove('softmax_batch')        # one frame: the batch softmax is the frame's
    for mk in mistakes:
        bad = R.bottleneck_statement(x, sd, stride=stride, mistake=mk)
        err = np.abs(bad - out).max()
        print('%s %s: off by %.3g (bound %.3g)' % (name, mk, err, bound))
        assert err > bound, (name, mk, err, bound)


# ------------------------------------------------------------------------------------------------ modules
def _expand(fixture, case):
    """tests/test_gconv_refs.py: _expand (the run-length form of resnext_modules.json)."""
    out = []
    for stage, first, count, t in case['runs']:
        sid, shapes = fixture['templates'][t]
        for i in range(first, first + count):
            out += [(('%s.%d.' % (stage, i) if stage else '') + suffix, tuple(shape)) for suffix, shape in zip(fixture['suffixes'][sid], shapes)]
    return out


def _tupled(kw):
    return {k: (_tupled(v) if isinstance(v, dict) else tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}


def test_module_keys_and_shapes_equal_the_references():
    fixture = json.load(open(os.path.join(GOLDEN, 'gcb_modules.json')))
    cases = fixture['cases']
    assert [c['cls'] for c in cases] == ['ResNet', 'ResNet', 'ResNeXt']
    for c in cases:
        net = build_from_cfg(dict(type=c['cls'], **_tupled(c['kwargs'])), BACKBONES)
        assert type(net) is getattr(hvrnet_amd, c['cls'])
        want = _expand(fixture, c)
        got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert got == want, (c['cls'], c['kwargs'], [p for p in zip(got, want) if p[0] != p[1]][:3])
        assert sum('context_block' in k for k, _ in got) > 0
        # strict round trip through randomised tensors of the fixture's shapes
        g = torch.Generator().manual_seed(1)
        sd = {k: (torch.randn(s, generator=g) if len(s) else torch.zeros((), dtype=torch.long)) for k, s in want}
        net.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())


def test_synthetic_state_dict_option():
    plain = S.synth_state_dict('hvr', depth=50)
    again = S.synth_state_dict('hvr', depth=50, gcb=None)
    assert list(plain) == list(again) and all(torch.equal(plain[k], again[k]) for k in plain)
    sd = S.synth_state_dict('hvr', depth=50, gcb=GCB)
    net = hvrnet_amd.ResNet(50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', gcb=GCB,
                            stage_with_gcb=(False, True, True))
    bsd = {k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.')}
    net.load_state_dict(bsd, strict=True)
    assert list(bsd) == list(net.state_dict())
    assert all(float(v.abs().max()) > 0 for k, v in bsd.items() if k.endswith('_conv.3.weight'))
    assert set(sd) - set(plain) == set('backbone.' + k for k in bsd if 'context_block' in k)


def test_context_block_assertions_and_initialisation():
    for bad in (dict(pooling_type='max'), dict(fusion_types='channel_add'), dict(fusion_types=('channel_sub', )), dict(fusion_types=())):
        with pytest.raises(AssertionError):
            ops.ContextBlock(64, 0.25, **bad)
    cb = ops.ContextBlock(64, 0.25, 'att', ('channel_add', 'channel_mul'))
    assert cb.planes == 16 and [k for k in cb.state_dict()] == [
        'conv_mask.weight', 'conv_mask.bias'] + ['channel_%s_conv.%d.%s' % (b, i, p) for b in ('add', 'mul') for i in (0, 1, 3) for p in ('weight', 'bias')]
    assert tuple(cb.channel_mul_conv[1].weight.shape) == (16, 1, 1) and tuple(cb.conv_mask.weight.shape) == (1, 64, 1, 1)
    for seq in (cb.channel_add_conv, cb.channel_mul_conv):
        assert float(seq[3].weight.detach().abs().max()) == 0 and float(seq[3].bias.detach().abs().max()) == 0 and float(seq[0].weight.detach().abs().max()) > 0
    assert float(cb.conv_mask.bias.detach().abs().max()) == 0 and cb.conv_mask.inited is True
    # kaiming, fan_in: std = sqrt(2 / 64) over 64 draws
    assert 0.5 * (2 / 64) ** 0.5 < float(cb.conv_mask.weight.detach().std()) < 1.5 * (2 / 64) ** 0.5
    avg = ops.ContextBlock(64, 0.25, 'avg', ['channel_mul'])
    assert not hasattr(avg, 'conv_mask') and avg.channel_add_conv is None and list(avg.state_dict())[0] == 'channel_mul_conv.0.weight'
    with pytest.raises(NotImplementedError):
        cb(torch.zeros((1, 64, 4, 4)))
    assert hvrnet_amd.ContextBlock is ops.ContextBlock


def test_routes_of_a_gcb_stage():
    kw = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
    net = hvrnet_amd.ResNet(50, gcb=GCB, stage_with_gcb=(False, False, True), **kw)
    plain = hvrnet_amd.ResNet(50, **kw)
    B, H, W = 3, 32, 40
    for dtype in (torch.bfloat16, torch.float16, hvrnet_amd.native.SPLIT, torch.float32):
        # the stages in front of the gcb stage keep their routes, compact ones included; the gcb stage runs at full resolution
        r0, r1 = net.stage_route(0, B, H, W, dtype), net.stage_route(1, B, *plain.stage_route(0, B, H, W, dtype).out_hw, dtype, plain.stage_route(0, B, H, W, dtype).compact)
        assert str(r0) == str(plain.stage_route(0, B, H, W, dtype))
        assert str(r1) == str(plain.stage_route(1, B, *r0.out_hw, dtype, r0.compact))
        r2 = net.stage_route(2, B, *r1.out_hw, dtype, r1.compact)
        assert [s.kind for s in r2.steps] == ['gcb'] * 6 and r2.steps[0].downsample and not any(s.downsample for s in r2.steps[1:])
        assert str(r2).startswith('downsample+gcb, gcb x5') and not r2.compact
    # a gcb stage is never compacted, and the stage in front of it still is (layer 1 ahead of a gcb layer 2)
    net2 = hvrnet_amd.ResNet(50, gcb=GCB, stage_with_gcb=(False, True, True), **kw)
    a, b = net2.stage_route(0, B, H, W, torch.bfloat16), plain.stage_route(0, B, H, W, torch.bfloat16)
    assert str(a) == str(b)
    r = net2.stage_route(1, B, *a.out_hw, torch.bfloat16, a.compact)
    assert [s.kind for s in r.steps] == ['gcb'] * 4 and not r.compact and not net2._dead_pixels(1) and plain._dead_pixels(1)


def test_refusals():
    kw = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    with pytest.raises(AssertionError):
        hvrnet_amd.ResNet(50, gcb=GCB, stage_with_gcb=(False, True, True, True), **kw)
    with pytest.raises(NotImplementedError):
        hvrnet_amd.Res2Net(gcb=GCB, stage_with_gcb=(False, True, True), **kw)
    with pytest.raises(NotImplementedError, match='marks no stage'):      # a gcb dict that no stage would use is refused, as before
        hvrnet_amd.ResNet(50, gcb=GCB, **kw, stage_with_gcb=(False, False, False))
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNet(50, gen_attention=dict(), **kw)
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNet(50, conv_cfg=dict(type='ConvWS'), **kw)
    with pytest.raises(TypeError):
        hvrnet_amd.ResLayer(50, gcb=GCB)
    blk = backbone.Bottleneck(64, 16, gcb=dict(ratio=0.25))
    assert blk.with_gcb and blk.context_block.inplanes == 64 and blk.context_block.fusion_types == ('channel_add', )
    with pytest.raises(NotImplementedError):
        blk.forward_train_nhwc(torch.zeros((1, 4, 4, 64)))
    both = backbone.Bottleneck(64, 16, gcb=dict(ratio=0.25), dcn=dict(modulated=False, deformable_groups=1))
    assert both.with_gcb and both.with_dcn
    grouped = backbone.Bottleneck(64, 64, groups=32, base_width=4, gcb=dict(ratio=0.25))
    assert grouped.with_gcb and grouped.groups == 32
