"""GPU tests of the ResNeXt path: the grouped 3x3 (native.conv3x3_grouped, both routes) against the f64 statement of
tests/gconv_refs.py in all four compute modes, the exact families (equality with round-to-nearest of the statement, grouped == dense
bit for bit), the refused shapes, grouped Bottlenecks against the hand-made chain of public native calls with every link held to
its statement, and a small ResNeXt + ResXLayer window eager / graphed."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import gconv_refs as G  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': SPLIT, 'f32': torch.float32}
NATIVE_MODES = ('bf16', 'f16')          # the modes gconv3x3.hip has instances for; f32 and split half run the dense route
GUARD_ROWS = 64
SENTINEL = 7777


def _run(c, geom, mode, route, relu=True):
    """native.conv3x3_grouped on true values (f64, CPU) into a sentinel-filled buffer with guard rows behind y.
    -> (stored values f64 [B, OH, OW, C] on the CPU, raw output tensor, guard rows untouched)"""
    B, H, W, C, Cg, s, d = geom
    x = D.to_device_operand(c['x'], mode, DEV)
    w = native.GroupedWeight(c['w'].float().to(DEV), DTYPES[mode])
    bias = c['bias'].float().to(DEV)
    OH, OW = G.out_hw(H, W, s)
    M = B * OH * OW
    buf = torch.full(((M + GUARD_ROWS) * C,), SENTINEL, dtype=DTYPES[mode], device=DEV)
    y = native.conv3x3_grouped(x, w, bias, relu, s, d, out=buf[:M * C].view(B, OH, OW, C), route=route)
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr()
    return F.values(y).cpu(), y, bool((buf[M * C:] == SENTINEL).all())


def _hold(got, c, geom, mode, what):
    B, H, W, C, Cg, s, d = geom
    ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, s, d)
    lo, hi = G.gconv_bracket(ref, mag, absxw, Cg, mode)
    ratio, bad, worst = F.compare(got, lo, hi, ref)
    print('%s %s %s: worst |got - ref| / bracket = %.3f, %d of %d outside' % (what, geom, mode, ratio, bad, ref.numel()))
    assert float(ref.abs().max()) > 0.5
    assert bad == 0, (what, geom, mode, ratio, bad, worst)


def _routes(mode):
    return ('grouped', 'dense', None) if mode in NATIVE_MODES else ('dense', None)


# ------------------------------------------------------------------------------------------------ kernel vs statement
@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('Cg', G.CGS)
def test_small_map_every_geometry(mode, Cg):
    """B = 2, 5 x 7, C = 64 (70 rows at stride 1, 24 at stride 2: a partly filled last pixel tile; two channel blocks and two pixel tiles
    per workgroup) over {stride 1, 2} x {dil 1, 2}, on every route the mode has."""
    for i, geom in enumerate(g for g in G.SMALL if g[4] == Cg):
        c = G.real_case(geom, mode, seed=200 + 10 * Cg + i)
        for route in _routes(mode):
            got, _, guard = _run(c, geom, mode, route)
            assert guard, 'guard rows behind y were written'
            _hold(got, c, geom, mode, 'route %s' % route)


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('geom', G.ODD + G.RES5, ids=lambda g: 'x'.join(str(v) for v in g))
def test_odd_rows_and_res5_shapes(mode, geom):
    """3 x 19 x 23 x 128 at Cg 4 (1 311 rows: no multiple of any tile, four channel blocks per workgroup; one tile per wave -- the waves that
    walk over several tiles are test_waves_that_walk_over_several_tiles);
    1 x 6 x 5 x 1024 at Cg 32, dilation 2 (res5's geometry: every tap of a border pixel leaves the map); 1 x 4 x 4 x 2048."""
    c = G.real_case(geom, mode, seed=300 + geom[3])
    got, _, guard = _run(c, geom, mode, None)
    assert guard
    _hold(got, c, geom, mode, 'automatic route')
    assert native.conv3x3_grouped_supported(geom[0], geom[1], geom[2], geom[3], geom[3] // geom[4], geom[5], geom[6], DTYPES[mode]) == (mode in NATIVE_MODES)


# (B, H, W, C, Cg, stride, dil): maps with more pixel tiles than the launch has wave slots, so that a wave runs its tile loop more than once --
# prefetch into the second register set, hand-over, next stride -- and SOME waves once more than others, the last tile partly filled.
# gconv3x3.hip, run_gconv3x3: a workgroup holds cbw = 4 channel blocks of 32 (C % 128 == 0) x 1 pixel tile, or cbw = 2 x 2 pixel tiles;
# grid.y = C / (32 cbw), grid.x = min(ceil(tiles cbw / 4), 2048 / grid.y); a wave walks over the tiles from its own in steps of grid.x 4 / cbw.
LOOPED = [(2, 129, 131, 128, 4, 1, 1),     # 33 798 rows = 2 113 tiles (6 rows in the last) on 2 048 slots, cbw 4, the two-taps-per-K-step form
          (3, 173, 169, 192, 16, 2, 1),    # stride 2 -> 22 185 rows = 1 387 tiles (9 rows) on 682 x 2 slots, cbw 2
          (1, 65, 65, 1024, 32, 1, 2),     # 4 225 rows = 265 tiles (1 row) on 256 slots, Cg 32, dilation 2
          (1, 46, 46, 2048, 32, 1, 1)]     # 2 116 rows = 133 tiles (4 rows) on 128 slots, the widest map


def _trips(geom):
    """(fewest, most) tiles any wave of the launch runs, by the rule quoted above."""
    B, H, W, C, Cg, s, d = geom
    OH, OW = G.out_hw(H, W, s)
    tiles = (B * OH * OW + 15) // 16
    cbw = 4 if C % 128 == 0 else 2
    gx = min((tiles * cbw + 3) // 4, max(1, 2048 // (C // (32 * cbw))))
    step = gx * (4 // cbw)
    return tiles // step, (tiles + step - 1) // step


@pytest.mark.parametrize('geom', LOOPED, ids=lambda g: 'x'.join(str(v) for v in g))
def test_waves_that_walk_over_several_tiles(geom):
    """The tile loop itself, in the two modes the kernel has (f32 and split half run the dense route: the tile engine, not this loop): on
    real operands every element inside its bracket; on exact operands the result equals round-to-nearest of the statement and the dense
    route bit for bit.  The f64 statements are evaluated on the device (a patch matrix of 0.3 GB)."""
    B, H, W, C, Cg, s, d = geom
    lo_trips, hi_trips = _trips(geom)
    assert lo_trips >= 1 and hi_trips == lo_trips + 1 and (B * G.out_hw(H, W, s)[0] * G.out_hw(H, W, s)[1]) % 16 != 0, (lo_trips, hi_trips)
    OH, OW = G.out_hw(H, W, s)
    M = B * OH * OW

    def run(c, mode, route):
        x = D.to_device_operand(c['x'], mode, DEV)
        w = native.GroupedWeight(c['w'].float().to(DEV), DTYPES[mode])
        buf = torch.full(((M + GUARD_ROWS) * C,), SENTINEL, dtype=DTYPES[mode], device=DEV)
        y = native.conv3x3_grouped(x, w, c['bias'].float().to(DEV), True, s, d, out=buf[:M * C].view(B, OH, OW, C), route=route)
        assert bool((buf[M * C:] == SENTINEL).all()), 'guard rows behind y were written'
        return y

    for mode in NATIVE_MODES:
        assert native.conv3x3_grouped_supported(B, H, W, C, C // Cg, s, d, DTYPES[mode])
        c = G.real_case(geom, mode, seed=500 + C, device=DEV)
        ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, s, d)
        lo, hi = G.gconv_bracket(ref, mag, absxw, Cg, mode)
        ratio, bad, worst = F.compare(F.values(run(c, mode, None)), lo, hi, ref)
        print('looped %s %s (%d - %d tiles per wave): worst / bracket = %.3f, %d of %d outside' % (geom, mode, lo_trips, hi_trips, ratio, bad, ref.numel()))
        assert bad == 0 and float(ref.abs().max()) > 0.5, (geom, mode, ratio, bad, worst)
        del ref, mag, absxw, lo, hi
    c = G.exact_gconv_case(geom, 'bf16', seed=600 + C, device=DEV)
    ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, s, d)
    F.assert_exact(c['x'], c['w'], mag, c['q'], 'bf16', ref)
    want = F.round_stored(ref, 'bf16')
    yg, yd = run(c, 'bf16', 'grouped'), run(c, 'bf16', 'dense')
    assert int((F.values(yg) != want).sum()) == 0 and torch.equal(yg, yd)
    first, last = yg.view(M, C)[:16], yg.view(M, C)[M - M % 16:]
    assert float(first.float().abs().max()) > 0 and float(last.float().abs().max()) > 0


def test_without_relu_and_with_a_fresh_output():
    geom = (2, 5, 7, 64, 8, 2, 1)
    c = G.real_case(geom, 'bf16', seed=5)
    ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], False, 2, 1)
    assert float(ref.min()) < -0.5
    lo, hi = G.gconv_bracket(ref, mag, absxw, 8, 'bf16')
    y = native.conv3x3_grouped(D.to_device_operand(c['x'], 'bf16', DEV), c['w'].float().to(DEV).bfloat16(), c['bias'].float().to(DEV), False, 2, 1)
    assert tuple(y.shape) == (2, 3, 4, 64) and F.compare(F.values(y).cpu(), lo, hi, ref)[1] == 0


# ------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize('mode', F.MODES)
def test_exact_sums_equal_the_rounded_statement_and_the_routes_each_other(mode):
    geoms = [g for g in G.SMALL if (g[5], g[6]) in ((1, 1), (2, 2))] + G.ODD + G.RES5[:1]
    for i, geom in enumerate(geoms):
        B, H, W, C, Cg, s, d = geom
        for family in G.exact_families(mode):
            c = G.exact_gconv_case(geom, mode, seed=400 + i, family=family)
            ref, mag, absxw = G.gconv_statement(c['x'], c['w'], c['bias'], True, s, d)
            F.assert_exact(c['x'], c['w'], mag, c['q'], mode, ref)
            want = F.round_stored(ref, mode) if mode != 'f32' else ref
            raws = []
            for route in _routes(mode):
                got, raw, guard = _run(c, geom, mode, route)
                assert guard
                nbad = int((got != want).sum())
                assert nbad == 0, (geom, mode, family, route, nbad)
                raws.append(raw.clone())
            assert all(torch.equal(raws[0], r) for r in raws[1:]), (geom, mode, family)


# ------------------------------------------------------------------------------------------------ refusals
def test_shapes_outside_the_instance_set_raise():
    def call(C, Cg, stride, dil, dtype=torch.bfloat16):
        x = torch.zeros((1, 6, 6, C), dtype=dtype, device=DEV)
        return native.conv3x3_grouped(x, torch.zeros((C, 3, 3, Cg), dtype=dtype, device=DEV), torch.zeros(C, device=DEV), True, stride, dil, route='grouped')
    assert tuple(call(64, 8, 1, 1).shape) == (1, 6, 6, 64)
    for args, word in (((128, 2, 1, 1), 'none of 4 / 8 / 16 / 32'), ((128, 64, 1, 1), 'none of 4 / 8 / 16 / 32'), ((64, 8, 3, 1), 'stride'),
                       ((96, 8, 1, 1), 'multiple of 64'), ((64, 8, 1, 3), 'pad')):
        with pytest.raises(native.HvrError, match=word):
            call(*args)
    with pytest.raises(native.HvrError, match='dense'):
        call(64, 8, 1, 1, torch.float32)
    with pytest.raises(native.HvrError, match='grouped form'):
        native.conv3x3_grouped(torch.zeros((1, 6, 6, 64), dtype=SPLIT, device=DEV), torch.zeros((64, 3, 3, 8), device=DEV), torch.zeros(64, device=DEV),
                               True, 1, 1, route='grouped')
    # pad != dil has no spelling in the wrapper: the C entry refuses it, with a message, before it launches anything
    x = torch.zeros((1, 6, 6, 64), dtype=torch.bfloat16, device=DEV)
    d = native.GConvDesc(x=x.data_ptr(), w=x.data_ptr(), y=x.data_ptr(), bias=x.data_ptr(), B=1, H=6, W=6, C=64, groups=8, stride=1, pad=2, dil=1,
                         relu=1, dtype=native.HVR_BF16)
    with pytest.raises(native.HvrError, match='pad == dil'):
        native._check(native.lib().hvr_conv3x3_grouped(ctypes.byref(d), None), 'hvr_conv3x3_grouped')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ modules vs the hand-made chain
def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (1.0 / fan) ** 0.5
            if m.bias is not None:
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_mean.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_var.data = torch.rand(m.bias.shape, generator=g) + 0.5
    return module


def _link(what, mode, got, ref, mag, absxw, K):
    lo, hi = F.stored_bracket(ref, F.mfma_bound(mag, absxw, K, mode), mode)
    ratio, bad, _ = F.compare(F.values(got), lo, hi, ref)
    print('  %-10s %s: worst / bracket = %.3f' % (what, mode, ratio))
    assert bad == 0, (what, mode, ratio, bad)


def _stored_grouped(gw, mode):
    """The values [C, 3, 3, Cg] of the operand conv2 reads: the grouped form where the kernel has one, else (and with mode 'dense') the
    diagonal blocks of the dense form -- whose every other entry must be an exact zero."""
    if mode in NATIVE_MODES:
        return F.values(gw.grouped(), 'weight')
    dv = F.values(gw.dense(), 'weight')
    n, Cg = gw.groups, gw.Cg
    i = torch.arange(n, device=dv.device)
    blocks = dv.view(n, Cg, 3, 3, n, Cg)[i, :, :, :, i, :]
    assert int((dv != 0).sum()) == int((blocks != 0).sum()) > 0
    return blocks.reshape(gw.C, 3, 3, Cg)


def _hand_block(blk, x, mode, route=None):
    """The grouped block's forward as public native calls on its packed weights (conv2 on `route`), each link checked against its
    statement on the operands it received."""
    p = blk.packed(x.device)
    V = F.values
    w1, b1 = p['c1']
    h1 = native.conv2d_nhwc(x, w1, b1, relu=True, stride=blk.conv1_stride)
    _link('conv1', mode, h1, *F.conv_statement(V(x), V(w1, 'weight'), b1, None, True, blk.conv1_stride, 0, 1), w1.shape[3])
    gw, b2 = p['c2']
    assert isinstance(gw, native.GroupedWeight) and gw.groups == blk.groups and gw.C == blk.width
    h2 = native.conv3x3_grouped(h1, gw, b2, True, blk.conv2_stride, blk.dilation, route=route)
    _link('conv2', mode, h2, *G.gconv_statement(V(h1), _stored_grouped(gw, mode if route is None else 'dense'), b2, True, blk.conv2_stride, blk.dilation), 9 * gw.Cg)
    w3, b3 = p['c3']
    if blk.downsample is not None and blk.fuse_tail and native.bottleneck_tail_supported(h2, x, p['tail'][0], p['tail'][1], blk.stride):
        y = native.bottleneck_tail(h2, x, p['tail'][0], p['tail'][1], stride2=blk.stride, relu=True)
        _link('tail', mode, y, *F.tail_statement(V(h2), V(x), V(p['tail'][0], 'weight'), p['tail'][1], blk.stride), p['tail'][0].shape[1])
        return y
    ident = x
    if blk.downsample is not None:
        wd, bd = p['ds']
        ident = native.conv2d_nhwc(x, wd, bd, relu=False, stride=blk.stride)
        _link('shortcut', mode, ident, *F.conv_statement(V(x), V(wd, 'weight'), bd, None, False, blk.stride, 0, 1), wd.shape[3])
    y = native.conv2d_nhwc(h2, w3, b3, resid=ident, relu=True)
    _link('conv3', mode, y, *F.conv_statement(V(h2), V(w3, 'weight'), b3, V(ident), True, 1, 0, 1), w3.shape[3])
    return y


def _act(shape, mode, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).clamp(min=0.0)
    return D.to_device_operand(F.store_true(x, mode), mode, DEV)


BLOCKS = [   # constructor keywords, with a projection, input [B, H, W, Cin]
    (dict(inplanes=256, planes=64, groups=32, base_width=4), False, (2, 10, 12, 256)),                              # layer 1 of 32x4d: width 128, Cg 4
    (dict(inplanes=256, planes=128, stride=2, groups=32, base_width=4, style='pytorch'), True, (2, 10, 12, 256)),   # a stride-2 3x3, Cg 8
    (dict(inplanes=512, planes=128, stride=2, groups=32, base_width=4, style='caffe'), True, (2, 10, 12, 512)),     # the stride on conv1
    (dict(inplanes=1024, planes=512, dilation=2, groups=32, base_width=4), True, (1, 6, 8, 1024)),                  # res5: width 1024, Cg 32
    (dict(inplanes=128, planes=32, groups=8, base_width=16), False, (2, 9, 11, 128)),                               # the golden block: width 64, Cg 8
]


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('case', range(len(BLOCKS)))
def test_grouped_bottleneck_equals_the_hand_made_chain(mode, case):
    kw, proj, shape = BLOCKS[case]
    kw = dict(kw)
    if proj:
        kw['downsample'] = torch.nn.Sequential(torch.nn.Conv2d(kw['inplanes'], 4 * kw['planes'], 1, stride=kw.get('stride', 1), bias=False),
                                               torch.nn.BatchNorm2d(4 * kw['planes']))
    blk = _randomise(backbone.Bottleneck(**kw), 61 + case).to(DEV).eval()
    backbone.set_compute_dtype(blk, DTYPES[mode])
    x = _act(shape, mode, 62 + case)
    with torch.no_grad():
        y = blk.forward_nhwc(x)
        want = _hand_block(blk, x, mode)
        assert torch.equal(y, want)
        assert float(F.values(y).abs().max()) > 0.1
        if mode in NATIVE_MODES:      # the forced dense route: the kernel was the automatic choice; forced away from it, the block is the
            p = blk.packed(x.device)  # hand-made chain with conv2 on the dense route, every link of that chain inside its own bracket
            assert p['c2'][0]._dense is None, 'the block-diagonal weight was built although the grouped kernel ran'
            backbone.Bottleneck.grouped_route = 'dense'
            try:
                yd = blk.forward_nhwc(x)
            finally:
                backbone.Bottleneck.grouped_route = None
            assert p['c2'][0]._dense is not None
            assert torch.equal(yd, _hand_block(blk, x, mode, route='dense'))


def test_golden_block_on_the_device_in_f32():
    """The reference's two f64 blocks (tests/golden/g21_resnext_block.npz) through this project's Bottleneck in f32 mode.  The bound, from the
    formats alone: each of the three links errs by at most (K + 3) u sum|x||w| with K <= 128 and u = 2^-24, the f32 rounding of the
    parameters adds u per factor, and sum|x||w| of a link is some tens of its output's scale: 3 x 131 x 6e-8 x 40 = 9.4e-4 -> 1e-3 of the
    output's largest value.  (A wrong group map errs by the scale itself.)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g21_resnext_block.npz'))
    for name, stride, dil in (('a', 2, 1), ('b', 1, 2)):
        down = torch.nn.Sequential(torch.nn.Conv2d(128, 128, 1, stride=2, bias=False), torch.nn.BatchNorm2d(128)) if name == 'a' else None
        blk = backbone.Bottleneck(128, 32, stride, dil, down, style='pytorch', groups=8, base_width=16)
        blk.load_state_dict({k[2:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith(name + '.') and k != name + '.out'}, strict=True)
        blk = blk.to(DEV).eval()
        backbone.set_compute_dtype(blk, torch.float32)
        with torch.no_grad():
            y = blk(torch.from_numpy(z['x']).float().to(DEV))
        want = torch.from_numpy(z[name + '.out'])
        assert tuple(y.shape) == tuple(want.shape)
        err = float((y.double().cpu() - want).abs().max())
        print('golden block %s in f32: max |y - ref| = %.3g of scale %.3g' % (name, err, float(want.abs().max())))
        assert err <= 1e-3 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ a ResNeXt window
HW, PAD = (120, 150), (128, 160)
T, NPROP = 3, 16


def _window_model(dtype):
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(type='ResNeXt', depth=50, groups=32, base_width=4, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1),
                              out_indices=(2,), style='pytorch', norm_eval=True)
    cfg.model.shared_head = dict(type='ResXLayer', depth=50, stage=3, stride=1, dilation=2, groups=32, base_width=4, style='pytorch', norm_eval=True,
                                 external_conv=True)
    return hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', depth=50, groups=32, base_width=4), dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_resnext_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert type(model.backbone).__name__ == 'ResNeXt' and type(model.shared_head).__name__ == 'ResXLayer'
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [torch.cat([S.synth_frame(10 * c + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV) for c in range(2)]
    with torch.no_grad():
        c4 = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
    assert tuple(c4.shape) == (T, 1024, 8, 10) and bool(torch.isfinite(c4.float()).all()) and float(c4.float().abs().max()) > 0
    first = [_eager(model, clip, metas) for clip in clips]
    again = [_eager(model, clip, metas) for clip in clips]
    g = GraphedClip(model, clips[0], metas, rescale=True)
    n_det = 0
    for rep in range(2):
        for clip, want, want2 in zip(clips, first, again):
            got = g.run(clip).result()
            assert len(got) == len(want) == 2
            assert all(_same(a, b) for a, b in zip(want, want2)), 'two eager calls differ'
            assert all(_same(a, b) for a, b in zip(got, want)), 'graph replay differs from the eager window'
            for dets in got[-1]:                      # per class: [n, 5] boxes + score, finite, scores in [0, 1], x1 <= x2, y1 <= y2
                a = np.asarray(dets)
                assert a.ndim == 2 and a.shape[1] == 5 and np.isfinite(a).all()
                assert (a[:, 4] >= 0).all() and (a[:, 4] <= 1).all() and (a[:, 0] <= a[:, 2]).all() and (a[:, 1] <= a[:, 3]).all()
                n_det += len(a)
    assert n_det > 0
