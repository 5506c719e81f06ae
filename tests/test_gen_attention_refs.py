"""CPU tests of the generalized attention block's statements (tests/gen_attention_refs.py), its fixtures made by running the reference
(tests/golden/make_gen_attention_golden.py) and the module surface: registry, keys, strict loading, initialisation, refusals, stage
routes, the synthetic weights and the kernel's shape query."""
import json
import os

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import backbone, native, ops, synthetic as S
from hvrnet_amd.registry import BACKBONES, build_from_cfg
from tests import gen_attention_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GA = dict(spatial_range=-1, num_heads=8, attention_type='1111', kv_stride=2)
# the constructor keywords of the fixtures' modules (make_gen_attention_golden.py)
BARE = dict(a=dict(in_dim=64, num_heads=8, kv_stride=2, attention_type='1111'), b=dict(in_dim=64, num_heads=8, kv_stride=2, attention_type='0010'),
            c=dict(in_dim=64, num_heads=8, kv_stride=2, attention_type='0011'), d=dict(in_dim=72, num_heads=9, kv_stride=1, attention_type='1001'),
            e=dict(in_dim=64, num_heads=8, kv_stride=2, attention_type='1011', position_embedding_dim=32, position_magnitude=2))
BLOCKS = dict(f=(dict(num_heads=4, kv_stride=2), 1), g=(dict(num_heads=2, kv_stride=2, attention_type='0111'), 2))


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1))).astype(np.float64)


def golden(name):
    z = np.load(os.path.join(GOLDEN, 'g24_gen_attention_blocks.npz' if name in BLOCKS else 'g24_gen_attention.npz'))
    sd = {k[len(name) + 1:]: z[k].astype(np.float64) for k in z.files if k.startswith(name + '.') and k.split('.')[-1] not in ('x', 'out', 'out_f32')}
    return sd, _nhwc(z[name + '.x']), _nhwc(z[name + '.out']), _nhwc(z[name + '.out_f32'])


# ------------------------------------------------------------------------------------------------ fixtures made by running the reference
def test_fixtures_are_small_and_hold_float32_parameters():
    for f in ('g24_gen_attention.npz', 'g24_gen_attention_blocks.npz', 'gen_attention_modules.json'):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f
    for f in ('g24_gen_attention.npz', 'g24_gen_attention_blocks.npz'):
        z = np.load(os.path.join(GOLDEN, f))
        for k in z.files:
            want = np.float64 if k.endswith('.out') else np.int64 if k.endswith('num_batches_tracked') else np.float32
            assert z[k].dtype == want, (k, z[k].dtype)
    for name in list(BARE) + list(BLOCKS):     # gamma and the biases carry values: no block is the identity
        sd = golden(name)[0]
        pre = 'gen_attention_block.' if name in BLOCKS else ''
        assert abs(float(sd[pre + 'gamma'][0])) >= 0.5 and np.abs(sd[pre + 'proj_conv.bias']).max() > 0
        assert all(np.abs(sd[pre + b]).max() > 0.5 for b in ('appr_bias', 'geom_bias') if pre + b in sd)


def _fixture_bound(out, out32):
    dist = np.abs(out32 - out).max()
    assert 1e-8 * np.abs(out).max() < dist < 1e-5 * np.abs(out).max()
    return R.FIXTURE_FACTOR * dist


@pytest.mark.parametrize('name', sorted(BARE))
def test_statement_reproduces_the_stand_alone_modules(name):
    sd, x, out, out32 = golden(name)
    prm = R.block_params(sd, BARE[name])
    assert prm['d'] == BARE[name]['in_dim'] // BARE[name]['num_heads'] and prm['t'] == R.bits(BARE[name]['attention_type'])
    r = R.block_statement(x, prm)
    bound = _fixture_bound(out, out32)
    err = np.abs(r['y'] - out).max()
    print('%s: |statement - fixture| max %.3g, bound %.3g (f32 run off by %.3g)' % (name, err, bound, bound / R.FIXTURE_FACTOR))
    assert r['y'].shape == out.shape and err <= bound
    # the reference's own f32 run sits inside the f32 block bound of the statement (the composite's rounding of a probability)
    assert R.outside(out32, r['y'], R.block_bound(x, prm, 'f32', r, p_round=R.U32)) == 0


@pytest.mark.parametrize('name', sorted(BLOCKS))
def test_statement_reproduces_the_bottlenecks(name):
    sd, x, out, out32 = golden(name)
    cfg, stride = BLOCKS[name]
    y = R.bottleneck_statement(x, sd, cfg, stride=stride)
    bound = _fixture_bound(out, out32)
    err = np.abs(y - out).max()
    print('%s: |statement - fixture| max %.3g, bound %.3g' % (name, err, bound))
    assert y.shape == out.shape and err <= bound
    assert np.abs(out32 - out).max() <= R.bottleneck_bound_f32(np.abs(out).max())


def test_every_named_mistake_leaves_the_bound_on_a_committed_case():
    """Each mistake against every fixture: it must leave the fixture's bound on at least one, or the cases are too weak."""
    seen = {mk: [] for mk in R.MISTAKES}
    for name in sorted(BARE) + sorted(BLOCKS):
        sd, x, out, out32 = golden(name)
        bound = _fixture_bound(out, out32)
        for mk in R.MISTAKES:
            if name in BLOCKS:
                bad = R.bottleneck_statement(x, sd, BLOCKS[name][0], stride=BLOCKS[name][1], mistake=mk)
            else:
                bad = R.block_statement(x, R.block_params(sd, BARE[name]), mk)['y']
            with np.errstate(invalid='ignore'):
                if not (np.abs(bad - out) <= bound).all():
                    seen[mk].append((name, float(np.nanmax(np.abs(bad - out)))))
    for mk, hits in seen.items():
        print('%-20s %s' % (mk, ', '.join('%s %.2g' % h for h in hits)))
        assert hits, 'no committed case sees the mistake %r' % mk
    # the structural mistakes are not rounding-sized: each moves some case by more than a hundredth of the output's scale
    for mk in set(R.MISTAKES) - {'no_max'}:
        assert max(e for _, e in seen[mk]) > 1e-2, mk


def test_core_bound_is_sharp_enough_to_see_the_core_mistakes():
    """On a kernel-test case in bf16: the bound is a small part of the output's scale, zero spread gives the one-rounding bound, and the
    mistakes made inside the core land outside it."""
    c = R.core_case(2, 2, 16, 7, 9, 2, '1111', 'bf16', 3)
    args = (c['q'], c['k'], c['v'], c['H'], c['W'], c['Hk'], c['Wk'])
    kw = dict(ab=c['ab'], px=c['px'], py=c['py'], gx=c['gx'], gy=c['gy'], qk=c['qk'])
    r = R.core_statement(*args, **kw)
    bound = R.core_bound(*args, r, 'bf16', **kw)
    assert bound.max() < 0.05 * np.abs(c['v']).max() and bound.min() > 0
    for mk in ('scaled', 'softmax_queries', 'px_by_y'):
        assert R.outside(R.core_statement(*args, **kw, mistake=mk)['o'], r['o'], bound) > 0, mk
    flat = dict(c, v=np.broadcast_to(c['v'][:, :1], c['v'].shape).copy())
    r2 = R.core_statement(flat['q'], flat['k'], flat['v'], *args[3:], **kw)
    b2 = R.core_bound(flat['q'], flat['k'], flat['v'], *args[3:], r2, 'bf16', **kw)
    assert np.abs(r2['o'] - flat['v'][:, :1]).max() < 1e-14
    assert (b2 <= R.STORE_REL['bf16'] * np.abs(r2['o']) * 1.001 + 1e-4 * np.abs(r2['o'])).all()   # one rounding (+ the f32 chains)


def test_overflow_family_needs_the_running_maximum():
    c = R.core_case(1, 2, 16, 9, 11, 1, '1010', 'bf16', 5, energy_scale=6.0)
    args = (c['q'], c['k'], c['v'], c['H'], c['W'], c['Hk'], c['Wk'])
    r = R.core_statement(*args, ab=c['ab'], qk=True)
    assert np.abs(r['E']).max() > 89.0        # exp of the largest energy overflows f32
    bad = R.core_statement(*args, ab=c['ab'], qk=True, mistake='no_max')['o']
    assert np.isfinite(r['o']).all() and R.outside(bad, r['o'], R.core_bound(*args, r, 'bf16', ab=c['ab'], qk=True)) > 0


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
    return {k: (_tupled(v) if isinstance(v, dict) else tuple(tuple(e) if isinstance(e, list) else e for e in v) if isinstance(v, list) else v)
            for k, v in kw.items()}


def test_module_keys_shapes_and_order_equal_the_references():
    fixture = json.load(open(os.path.join(GOLDEN, 'gen_attention_modules.json')))
    assert [c['kwargs']['depth'] for c in fixture['cases']] == [50, 101]
    for c in fixture['cases']:
        kw = _tupled(c['kwargs'])
        assert kw['stage_with_gen_attention'] == ((), (), (0, 2, 5), (0, 1, 2))
        net = build_from_cfg(dict(type='ResNet', **kw), BACKBONES)
        assert type(net) is hvrnet_amd.ResNet
        want = _expand(fixture, c)
        got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert got == want, (c['kwargs'], [p for p in zip(got, want) if p[0] != p[1]][:3])
        assert sorted(set(k.split('.gen_attention_block')[0] for k, _ in got if 'gen_attention_block' in k)) == \
            ['layer3.0', 'layer3.2', 'layer3.5', 'layer4.0', 'layer4.1', 'layer4.2']
        g = torch.Generator().manual_seed(1)
        sd = {k: (torch.randn(s, generator=g) if len(s) else torch.zeros((), dtype=torch.long)) for k, s in want}
        net.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    types = []
    for b in fixture['bare']:
        m = ops.GeneralizedAttention(**b['kwargs'])
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == b['keys'], b['kwargs']
        types.append(b['kwargs']['attention_type'])
    assert types[:len(R.TYPES)] == list(R.TYPES)
    assert hvrnet_amd.GeneralizedAttention is ops.GeneralizedAttention


def test_initialisation_is_the_references():
    m = ops.GeneralizedAttention(256, num_heads=8, attention_type='1111')
    assert m.qk_embed_dim == 32 and float(m.gamma.detach()) == 0.0 and float(m.proj_conv.bias.detach().abs().max()) == 0.0
    for mod, fan in ((m.query_conv, 256), (m.key_conv, 256), (m.value_conv, 256), (m.proj_conv, 256), (m.appr_geom_fc_x, 128), (m.appr_geom_fc_y, 128)):
        w, lim = mod.weight.detach(), (3.0 / fan) ** 0.5           # kaiming-uniform, a = 1, fan_in
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.95 * lim and abs(float(w.std()) - lim / 3 ** 0.5) < 0.05 * lim
    for b in (m.appr_bias, m.geom_bias):
        lim = 1.0 / (2 * 32) ** 0.5
        assert tuple(b.shape) == (256,) and float(b.detach().abs().max()) <= lim and float(b.detach().abs().max()) > 0.9 * lim
    nine = ops.GeneralizedAttention(256)                             # the default nine heads: 9 x 28 = 252 of 256 channels
    assert nine.qk_embed_dim == 28 and tuple(nine.query_conv.weight.shape) == (252, 256, 1, 1) and tuple(nine.proj_conv.weight.shape) == (256, 252, 1, 1)
    only_key = ops.GeneralizedAttention(64, num_heads=8, attention_type='0010')
    assert list(only_key.state_dict()) == ['appr_bias', 'gamma', 'key_conv.weight', 'value_conv.weight', 'proj_conv.weight', 'proj_conv.bias']
    with pytest.raises(NotImplementedError):
        m(torch.zeros((1, 256, 4, 4)))
    with pytest.raises(NotImplementedError):
        m.forward_nhwc(torch.zeros((1, 4, 4, 256)))


def test_position_tables_are_the_statements_and_cached():
    sd, x, _, _ = golden('e')
    m = ops.GeneralizedAttention(**BARE['e'])
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=True)
    backbone.set_compute_dtype(m, torch.float32)
    t = m.position_tables(6, 5, torch.device('cpu'))
    prm = R.block_params(sd, BARE['e'])
    px, py = R.position_tables(prm, 6, 5)
    assert set(t) == {'gx', 'gy'}                                   # '1011': no query x position term, the tables enter through geom_bias only
    gb = R.split_heads(prm['gb'], 8)[:, None, None, :]
    assert np.abs(t['gx'].double().numpy() - (px * gb).sum(3)).max() < 1e-6 and np.abs(t['gy'].double().numpy() - (py * gb).sum(3)).max() < 1e-6
    assert m.position_tables(6, 5, torch.device('cpu')) is t and m.position_tables(5, 6, torch.device('cpu')) is not t
    m.load_state_dict(m.state_dict())                                # the tables go with the packed weights
    assert m.position_tables(6, 5, torch.device('cpu')) is not t
    full = ops.GeneralizedAttention(**BARE['a'])
    backbone.set_compute_dtype(full, torch.bfloat16)
    tf = full.position_tables(5, 7, torch.device('cpu'))
    assert tf['px'].dtype == torch.bfloat16 and tuple(tf['px'].shape) == (8, 7, 4, 8) and tuple(tf['py'].shape) == (8, 5, 3, 8)
    assert tf['gx'].dtype == torch.float32 and tuple(tf['gx'].shape) == (8, 7, 4)


def test_refusals():
    for t in R.REFUSED_TYPES:
        with pytest.raises(NotImplementedError, match='transposed'):
            ops.GeneralizedAttention(64, num_heads=8, attention_type=t)
    for t in R.TYPES:
        ops.GeneralizedAttention(64, num_heads=8, attention_type=t)
    with pytest.raises(NotImplementedError, match='q_stride'):
        ops.GeneralizedAttention(64, num_heads=8, q_stride=2)
    with pytest.raises(NotImplementedError, match='spatial_range'):
        ops.GeneralizedAttention(256, num_heads=8, spatial_range=2)
    kw = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    with pytest.raises(ValueError, match='names block'):
        hvrnet_amd.ResNet(50, gen_attention=GA, stage_with_gen_attention=((), (4,), ()), **kw)          # layer 2 of R-50 has blocks 0 .. 3
    with pytest.raises(NotImplementedError, match='marks no block'):
        hvrnet_amd.ResNet(50, gen_attention=GA, **kw)
    with pytest.raises(NotImplementedError, match='marks no block'):
        hvrnet_amd.ResNet(50, gen_attention=GA, stage_with_gen_attention=((), (), (), (0,)), **kw)     # the only mark is past num_stages
    with pytest.raises(NotImplementedError):
        hvrnet_amd.ResNet(50, conv_cfg=dict(type='ConvWS'), **kw)
    with pytest.raises(NotImplementedError):
        hvrnet_amd.Res2Net(gen_attention=GA, stage_with_gen_attention=((), (1,), ()), **kw)
    for groups in (1, 32):
        with pytest.raises(NotImplementedError, match='ResNeXt'):
            hvrnet_amd.ResNeXt(depth=50, groups=groups, gen_attention=GA, stage_with_gen_attention=((), (1,), ()), **kw)
    with pytest.raises(NotImplementedError, match='grouped'):
        backbone.Bottleneck(256, 64, groups=32, gen_attention=dict(num_heads=4))
    for cls in (hvrnet_amd.ResLayer, hvrnet_amd.ResXLayer):
        with pytest.raises(TypeError):
            cls(50, gen_attention=GA)
    # longer than num_stages is fine (the default has four entries), and inference only
    net = hvrnet_amd.ResNet(50, gen_attention=GA, stage_with_gen_attention=((), (1,), (0, 5), (0, 1, 2)), **kw)
    assert [[b.with_gen_attention for b in getattr(net, n)] for n in net.res_layers] == [[False] * 3, [False, True, False, False], [True] + [False] * 4 + [True]]
    assert net.layer2[1].gen_attention_block.channel_in == 128 and net.layer3[0].gen_attention_block.qk_embed_dim == 32
    with pytest.raises(NotImplementedError, match='inference only'):
        net.forward_train_nhwc(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(NotImplementedError, match='inference only'):
        net.layer2[1].forward_train_nhwc(torch.zeros((1, 4, 4, 512)))


def test_detectors_refuse_to_train_through_attention_blocks():
    """HNMBRCNN.forward_train runs the backbone frozen, under no_grad, and would never reach the backbone's own refusal: the detectors'
    training entries refuse such a backbone themselves, before anything runs."""
    from hvrnet_amd.config import hvr_config, selsa_config
    from hvrnet_amd.registry import build_detector
    for make in (hvr_config, selsa_config):
        cfg = make(frame_interval=1, nms_post=16)
        cfg.model.backbone = dict(cfg.model.backbone, depth=50, gen_attention=GA, stage_with_gen_attention=((), (), (0,)))
        cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
        model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        with pytest.raises(NotImplementedError, match='inference only'):
            model.forward_train(torch.zeros((9, 3, 64, 64)), [{}] * 9, [], [])
        if hasattr(model, 'forward_train_sampled'):
            with pytest.raises(NotImplementedError, match='inference only'):
                model.forward_train_sampled(torch.zeros((3, 3, 64, 64)), None, None, None, None, None, None)


def test_routes_of_a_stage_with_attention_blocks():
    kw = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
    plain = hvrnet_amd.ResNet(50, **kw)
    net = hvrnet_amd.ResNet(50, gen_attention=GA, stage_with_gen_attention=((), (1,), (0, 5)), **kw)
    B, H, W = 15, 152, 252
    for dtype in (torch.bfloat16, torch.float16, native.SPLIT, torch.float32):
        p0, p1 = plain.stage_route(0, B, H, W, dtype), None
        p1 = plain.stage_route(1, B, *p0.out_hw, dtype, p0.compact)
        p1_full = hvrnet_amd.ResNet(50, **dict(kw, out_indices=(1, 2))).stage_route(1, B, *p0.out_hw, dtype, p0.compact)   # layer 2 kept whole: not compacted
        r0 = net.stage_route(0, B, H, W, dtype)
        assert str(r0) == str(p0)                                   # the stage in front is still compacted
        r1 = net.stage_route(1, B, *r0.out_hw, dtype, r0.compact)
        assert not r1.compact and not net._dead_pixels(1) and not net._ends_compact(1)
        assert not any(s.kind in ('close_sampled', 'tail_next_live') or s.compact for s in r1.steps)
        assert str(r1) == str(p1_full)                              # the body's output is all a close reads: the fused closes stay
        r2 = net.stage_route(2, B, *r1.out_hw, dtype, r1.compact)
        assert str(r2) == str(plain.stage_route(2, B, *r1.out_hw, dtype, False))
    p0 = plain.stage_route(0, B, H, W, torch.bfloat16)
    assert p0.compact and str(net.stage_route(0, B, H, W, torch.bfloat16)) == str(p0)
    assert plain._dead_pixels(0) and net._dead_pixels(0) and plain._dead_pixels(1)
    bf = net.stage_route(1, B, *p0.out_hw, torch.bfloat16, True)
    assert {s.kind for s in bf.steps} & {'tail', 'tail_next'}, str(bf)
    # a model without attention blocks plans what it planned before
    assert str(plain.stage_route(0, 3, 32, 40, torch.bfloat16)) == 'tail_next(projection), tail_next_live, close_sampled/1 -> 16x20 compact'


def test_synthetic_state_dict_option():
    plain = S.synth_state_dict('hvr', depth=50)
    again = S.synth_state_dict('hvr', depth=50, gen_attention=None)
    assert list(plain) == list(again) and all(torch.equal(plain[k], again[k]) for k in plain)
    swa = ((), (1,), (0, 5))
    sd = S.synth_state_dict('hvr', depth=50, gen_attention=GA, stage_with_gen_attention=swa)
    net = hvrnet_amd.ResNet(50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', gen_attention=GA,
                            stage_with_gen_attention=swa)
    bsd = {k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.')}
    net.load_state_dict(bsd, strict=True)
    assert set(sd) - set(plain) == set('backbone.' + k for k in bsd if 'gen_attention_block' in k) and len(set(sd) - set(plain)) == 3 * 10
    for k, v in bsd.items():      # gamma and the biases are non-zero: the block is not the identity
        if k.endswith(('.gamma', '.appr_bias', '.geom_bias', 'gen_attention_block.proj_conv.bias')):
            assert float(v.abs().max()) > 0, k


def test_shape_query_and_routes_of_the_core():
    bf, hf = torch.bfloat16, torch.float16
    assert all(native.gen_attn_supported(d, h, 19, 32, dt) for d in (16, 32, 64) for h in (1, 8, 9) for dt in (bf, hf))
    assert not any(native.gen_attn_supported(d, 8, 19, 32, bf) for d in (8, 24, 28, 48, 128))
    assert not native.gen_attn_supported(32, 8, 19, 32, torch.float32) and not native.gen_attn_supported(32, 8, 19, 32, native.SPLIT)
    assert native.gen_attn_supported(16, 8, 38, 63, bf) and native.gen_attn_supported(16, 8, 256, 256, bf) and not native.gen_attn_supported(16, 8, 256, 257, bf)
    qt, kb = native.gen_attn_tiles()
    assert qt % 16 == 0 and kb % 16 == 0
    assert native.gen_attn_route(32, 8, 38, 63, 19, 32, torch.float32) == 'composite' and native.gen_attn_route(28, 9, 38, 63, 19, 32, bf) == 'composite'
    assert native.gen_attn_route(16, 1, 8, 8, 4, 4, bf, channels=64) == 'composite'      # zero-padded maps
    assert native.gen_attn_route(32, 8, 38, 63, 19, 32, bf, route='composite') == 'composite'
    assert native.gen_attn_route(32, 8, 5, 7, 3, 4, hf) in ('kernel', 'composite')        # by the measured table
    with pytest.raises(native.HvrError, match='no kernel'):
        native.gen_attn_route(28, 9, 38, 63, 19, 32, bf, route='kernel')
    for shape in native.GEN_ATTN_COMPOSITE_SHAPES:
        assert len(shape) == 6
    assert 64 << 20 <= native.GEN_ATTN_ENERGY_CAP <= 512 << 20
