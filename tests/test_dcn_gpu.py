"""GPU tests of the deformable-conv path: the sampler (hvr_deform_im2col) against the f64 statement of tests/dcn_refs.py in all
four compute modes, the exact families (equality with round-to-nearest of the statement), deform_conv2d_nhwc (chunking, the
zero-offset case inside the plain conv's bracket), dcn modules against the hand-made chain of public native calls with every link
held to its statement, dead-pixel compaction beside a dcn stage, and a dcn window eager / graphed / against the dcn-free model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, parity, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': SPLIT, 'f32': torch.float32}
GUARD_ROWS = 64
SENTINEL = 7777


def _sample(x_true, om, s, p, d, dg, mod, mode):
    """Runs the sampler on true values x (f64, CPU) and om (f32, CPU) into a sentinel-filled buffer with guard rows behind col.
    -> (stored values f64 on the CPU, guard rows untouched)"""
    xd = D.to_device_operand(x_true, mode, DEV)
    omd = om.to(DEV).contiguous()
    B, H, W, C = xd.shape
    OH, OW = D.out_hw(H, W, 3, 3, s, p, d)
    M, K = B * OH * OW, 9 * C
    buf = torch.full(((M + GUARD_ROWS) * K,), SENTINEL, dtype=DTYPES[mode], device=DEV)
    col = native.deform_im2col(xd, omd, 3, 3, s, p, d, dg, mod, out=buf[:M * K].view(M, K))
    torch.cuda.synchronize()
    return F.values(col).cpu(), bool((buf[M * K:] == SENTINEL).all())


def _hold(got, ref, bound, mode, what):
    lo, hi = D.stored_bracket(ref, bound, mode)
    ratio, bad, worst = F.compare(got, lo, hi, ref)
    print('%s %s: worst |got - ref| / bracket = %.3f, %d of %d outside' % (what, mode, ratio, bad, ref.numel()))
    assert bad == 0, (what, mode, ratio, bad, worst)


# ------------------------------------------------------------------------------------------------ sampler vs statement
SMALL = [(dg, spd, mod) for dg in (1, 2, 4) for spd in ((1, 1, 1), (1, 2, 2), (2, 1, 1)) for mod in (False, True)]


@pytest.mark.parametrize('mode', F.MODES)
def test_sampler_small_map_every_configuration(mode):
    """B = 2, 5 x 7, Cin = 64 (70 rows: less than one workgroup's share): groups 1 / 2 / 4, the three geometries, v1 and v2, with a
    row pitch of om larger than its channel count."""
    for i, (dg, (s, p, d), mod) in enumerate(SMALL):
        n = (3 if mod else 2) * dg * 9
        x, om = D.real_inputs(2, 5, 7, 64, 3, 3, s, p, d, dg, mod, mode, seed=100 + i, ldo=n + 3)
        ref, bound = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
        got, guard = _sample(x, om, s, p, d, dg, mod, mode)
        assert guard, 'guard rows behind col were written'
        assert float(ref.abs().max()) > 0.5
        _hold(got, ref, bound, mode, 'dg %d s%d p%d d%d mod %d' % (dg, s, p, d, mod))


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('shape', [(3, 19, 23, 128, 2, 1, 1, 1), (1, 6, 5, 512, 1, 1, 2, 2)])
def test_sampler_many_rows_and_wide_channels(mode, shape):
    """3 x 19 x 23 at Cin = 128 (1 311 rows: no multiple of any tile, several workgroups) and Cin = 512 with one group at res5's
    geometry (dilation 2)."""
    B, H, W, C, dg, s, p, d = shape
    for mod in (False, True):
        x, om = D.real_inputs(B, H, W, C, 3, 3, s, p, d, dg, mod, mode, seed=7, ldo=3 * dg * 9 + 1)
        ref, bound = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
        got, guard = _sample(x, om, s, p, d, dg, mod, mode)
        assert guard
        _hold(got, ref, bound, mode, '%dx%dx%dx%d mod %d' % (B, H, W, C, mod))


def test_bad_shapes_are_refused_with_a_message():
    x = torch.zeros((1, 4, 4, 48), dtype=torch.bfloat16, device=DEV)
    om = torch.zeros((1, 4, 4, 18), device=DEV)
    with pytest.raises(native.HvrError, match='K-step'):
        native.deform_im2col(x, om, 3, 3, 1, 1, 1, 1, False)
    x = torch.zeros((1, 4, 4, 64), dtype=torch.bfloat16, device=DEV)
    om = torch.zeros((1, 4, 4, 16 * 18), device=DEV)
    with pytest.raises(native.HvrError, match='8 channels per group'):
        native.deform_im2col(x, om, 3, 3, 1, 1, 1, 16, False)
    with pytest.raises(native.HvrError, match='ldo'):
        native.deform_im2col(x, torch.zeros((1, 4, 4, 18), device=DEV), 3, 3, 1, 1, 1, 1, True)
    assert native.lib().hvr_deform_im2col_supported(64, 2, native.HVR_BF16) == 1
    assert native.lib().hvr_deform_im2col_supported(48, 1, native.HVR_BF16) == 0
    assert native.lib().hvr_deform_im2col_supported(64, 16, native.HVR_F16S) == 0


# ------------------------------------------------------------------------------------------------ exact families
# ('lo_act': wide values with a non-zero lo half exist in the split-half format only)
@pytest.mark.parametrize('mode,family', [(m, f) for m in F.MODES for f in ('zero', 'integer', 'eighths', 'border')] + [('f16x2', 'lo_act')])
def test_exact_families_equal_the_rounded_statement(mode, family):
    for (B, H, W, C, dg) in ((2, 5, 7, 64, 2), (3, 19, 23, 128, 1)):
        for mod in (False, True):
            for (s, p, d) in ((1, 1, 1), (2, 1, 1), (1, 2, 2)):
                if (H, s) == (19, 2) or (H, d) == (19, 2):
                    continue                                    # (the larger map once: geometry is covered by the small one)
                x, om = D.exact_inputs(B, H, W, C, 3, 3, s, p, d, dg, mod, mode, seed=21, family=family, ldo=3 * dg * 9 + 2)
                ref, _ = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
                want = F.round_stored(ref.float().double(), mode)
                got, guard = _sample(x, om, s, p, d, dg, mod, mode)
                assert guard
                nbad = int((got != want).sum())
                assert nbad == 0, (family, mode, (B, H, W, C, dg), mod, (s, p, d), nbad)
                if family == 'zero' and not mod:
                    cols, _, _ = F._patches(x, 3, 3, s, p, d)
                    assert torch.equal(got, cols)
                if family == 'lo_act':
                    assert bool((F.split_parts(want, F.ACT_SCALE)[1] != 0).any())


# ------------------------------------------------------------------------------------------------ deform_conv2d_nhwc
def _conv_operands(B, H, W, Cin, Cout, mode, seed):
    a, w = F.real_operands((B, H, W, Cin), (Cout, 3, 3, Cin), mode, seed)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(seed + 1))
    wd = w.float().to(DEV)
    wd = native.as_operand(wd, SPLIT) if mode == 'f16x2' else wd.to(DTYPES[mode])
    return a, w, bias, D.to_device_operand(a, mode, DEV), wd, bias.to(DEV)


@pytest.mark.parametrize('mode', F.MODES)
def test_deform_conv_chunked_equals_unchunked_bit_for_bit(mode):
    B, H, W, Cin, Cout = 5, 10, 12, 64, 64
    a, w, bias, xd, wd, bd = _conv_operands(B, H, W, Cin, Cout, mode, 31)
    _, om = D.real_inputs(B, H, W, Cin, 3, 3, 1, 1, 1, 2, True, mode, seed=32)
    omd = om.to(DEV)
    whole = native.deform_conv2d_nhwc(xd, omd, wd, bd, True, 1, 1, 1, 2, True, chunk_rows=0)
    for rows in (H * W, 2 * H * W + 5, 4 * H * W):                   # chunks of 1, 2 and 4 frames (the last one shorter)
        part = native.deform_conv2d_nhwc(xd, omd, wd, bd, True, 1, 1, 1, 2, True, chunk_rows=rows)
        assert torch.equal(part, whole), rows
    with native.fewrow_split(True):                                  # the few-row K-sliced route stays off inside
        assert torch.equal(native.deform_conv2d_nhwc(xd[:1], omd[:1], wd, bd, True, 1, 1, 1, 2, True), whole[:1])
    assert float(F.values(whole).abs().max()) > 0.1


@pytest.mark.parametrize('mode', F.MODES)
def test_deform_conv_with_zero_offsets_lies_in_the_plain_conv_bracket(mode):
    for (s, p, d) in ((1, 1, 1), (1, 2, 2), (2, 1, 1)):
        B, H, W, Cin, Cout = 2, 9, 11, 64, 32
        a, w, bias, xd, wd, bd = _conv_operands(B, H, W, Cin, Cout, mode, 41)
        OH, OW = D.out_hw(H, W, 3, 3, s, p, d)
        omd = torch.zeros((B, OH, OW, 20), device=DEV)
        y = native.deform_conv2d_nhwc(xd, omd, wd, bd, True, s, p, d, 1, False)
        ref, mag, absxw = F.conv_statement(a, w, bias, None, True, s, p, d)
        lo, hi = F.stored_bracket(ref, F.mfma_bound(mag, absxw, 9 * Cin, mode), mode)
        ratio, bad, _ = F.compare(F.values(y).cpu(), lo, hi, ref)
        print('zero-offset deform conv %s s%d p%d d%d: worst / bracket = %.3f' % (mode, s, p, d, ratio))
        assert bad == 0


@pytest.mark.parametrize('mode,family', [(m, 'plain') for m in F.MODES] + [('f16x2', 'lo_act'), ('f16x2', 'lo_weight')])
def test_deform_conv_exact_sums_equal_the_rounded_statement(mode, family):
    """Zero offsets on the conv descriptors' exact-sum operands (split half: the two cross-term families): the sampler is an exact
    copy and every partial sum of the product is an f32 number, so the result must EQUAL round-to-nearest of the conv statement."""
    B, H, W, Cin, Cout = 2, 6, 7, 64, 32
    c = F.exact_case((B, H, W, Cin), (Cout, 3, 3, Cin), mode, 51, family=family)
    ref, mag, _ = F.conv_statement(c['a'], c['w'], c['bias'], None, True, 1, 1, 1)
    F.assert_exact(c['a'], c['w'], mag, c['q'], mode, ref)
    xd = D.to_device_operand(c['a'], mode, DEV)
    wd = c['w'].float().to(DEV)
    wd = native.as_operand(wd, SPLIT) if mode == 'f16x2' else wd.to(DTYPES[mode])
    omd = torch.zeros((B, H, W, 18), device=DEV)
    y = native.deform_conv2d_nhwc(xd, omd, wd, c['bias'].float().to(DEV), True, 1, 1, 1, 1, False)
    want = F.round_stored(ref, mode) if mode != 'f32' else ref
    assert torch.equal(F.values(y).cpu(), want)


# ------------------------------------------------------------------------------------------------ modules vs the hand-made chain
def _randomise(module, seed, offset_std=0.02):
    g = torch.Generator().manual_seed(seed)
    for name, m in module.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            std = offset_std if name.endswith('conv2_offset') else (1.0 / fan) ** 0.5
            m.weight.data = torch.randn(m.weight.shape, generator=g) * std
            if m.bias is not None:
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_mean.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_var.data = torch.rand(m.bias.shape, generator=g) + 0.5
    return module


def _link(what, mode, got, ref, mag, absxw, K, out_f32=False):
    lo, hi = F.stored_bracket(ref, F.mfma_bound(mag, absxw, K, mode), mode, out_f32)
    ratio, bad, _ = F.compare(got.double() if out_f32 else F.values(got), lo, hi, ref)
    print('  %-10s %s: worst / bracket = %.3f' % (what, mode, ratio))
    assert bad == 0, (what, mode, ratio, bad)


def _hand_block(blk, x, mode):
    """The block's forward as public native calls on its packed weights, each link checked against its statement on the operands
    it received."""
    p = blk.packed(x.device)
    s2, dil, dg, mod = blk.conv2_stride, blk.dilation, blk.deformable_groups, blk.with_modulated_dcn
    V = F.values
    w1, b1 = p['c1']
    h1 = native.conv2d_nhwc(x, w1, b1, relu=True, stride=blk.conv1_stride)
    _link('conv1', mode, h1, *F.conv_statement(V(x), V(w1, 'weight'), b1, None, True, blk.conv1_stride, 0, 1), w1.shape[3])
    wo, bo = p['off']
    om = native.conv2d_nhwc(h1, wo, bo, relu=False, stride=s2, pad=dil, dil=dil, out_f32=True)
    assert om.dtype == torch.float32 and om.shape[3] % 4 == 0 and om.shape[3] >= (27 if mod else 18) * dg
    _link('offsets', mode, om, *F.conv_statement(V(h1), V(wo, 'weight'), bo, None, False, s2, dil, dil), 9 * wo.shape[3], out_f32=True)
    col = native.deform_im2col(h1, om, 3, 3, s2, dil, dil, dg, mod)
    ref, bound = D.sampler_statement(V(h1), om, 3, 3, s2, dil, dil, dg, mod)           # the device's own offsets
    _hold(V(col).cpu(), ref, bound, mode, '  sampler')
    w2, b2 = p['c2']
    Cout = w2.shape[0]
    h2 = native.gemm(col, w2.reshape(Cout, -1), b2, relu=True)
    _link('product', mode, h2, *F.gemm_statement(V(col), V(w2, 'weight').reshape(Cout, -1), b2, None, True), col.shape[1])
    B, OH, OW = om.shape[:3]
    h2 = h2.view(B, OH, OW, Cout)
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


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('dcn', [dict(modulated=False, deformable_groups=1), dict(modulated=True, deformable_groups=2)])
def test_dcn_bottleneck_equals_the_hand_made_chain(mode, dcn):
    blk = _randomise(backbone.Bottleneck(256, 64, dcn=dcn), 61).to(DEV).eval()
    backbone.set_compute_dtype(blk, DTYPES[mode])
    x = _act((2, 10, 12, 256), mode, 62)
    with torch.no_grad():
        y = blk.forward_nhwc(x)
        want = _hand_block(blk, x, mode)
    assert torch.equal(y, want)
    assert float(F.values(y).abs().max()) > 0.1


@pytest.mark.parametrize('mode', F.MODES)
def test_dcn_res_layer_equals_the_hand_made_chain(mode):
    dcn = dict(modulated=True, deformable_groups=1, fallback_on_stride=False)
    head = _randomise(backbone.ResLayer(depth=50, stage=3, stride=1, dilation=2, style='caffe', dcn=dcn), 71).to(DEV).eval()
    backbone.set_compute_dtype(head, DTYPES[mode])
    x = _act((1, 6, 8, 1024), mode, 72)
    with torch.no_grad():
        y = backbone.as_nhwc(head(backbone.as_logical(x)), DTYPES[mode])
        want = x
        for blk in head.layer4:
            want = _hand_block(blk, want, mode)
    assert tuple(y.shape) == (1, 6, 8, 2048) and torch.equal(y, want)


def test_dcn_stage_next_to_dead_pixel_compaction_gives_the_same_c4():
    dcn = dict(modulated=True, deformable_groups=1, fallback_on_stride=False)
    net = backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', dcn=dcn,
                          stage_with_dcn=(False, False, True), zero_init_residual=False)
    _randomise(net, 81).to(DEV).eval()
    img = S.synth_frame(3, img_hw=(60, 90), pad_hw=(64, 96)).to(DEV)
    with torch.no_grad():
        assert net._ends_compact(0)
        a = net(img)[0].clone()
        backbone.ResNet.skip_dead_pixels = False
        try:
            assert not net._ends_compact(0)
            b = net(img)[0].clone()
        finally:
            backbone.ResNet.skip_dead_pixels = True
    assert tuple(a.shape) == (1, 1024, 4, 6) and torch.equal(a, b) and float(a.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ a dcn window
HW, PAD = (150, 250), (160, 256)
T, NPROP = 3, 24


def _window_model(dcn, dtype, offsets):
    """HNMBRCNN at depth 50 with synthetic weights; dcn in layer 3 and res5 when `dcn` is given.  offsets: 'zero' or 'random'."""
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone['depth'] = 50
    cfg.model.shared_head['depth'] = 50
    sd = S.synth_state_dict('hvr', depth=50)
    if dcn is not None:
        cfg.model.backbone['dcn'] = dcn
        cfg.model.backbone['stage_with_dcn'] = (False, False, True)
        cfg.model.shared_head['dcn'] = dcn
        g = torch.Generator().manual_seed(91)
        n = dcn['deformable_groups'] * (27 if dcn['modulated'] else 18)
        for prefix, planes, blocks in (('backbone.layer3', 256, 6), ('shared_head.layer4', 512, 3)):
            for i in range(blocks):
                k = '%s.%d.conv2_offset.' % (prefix, i)
                std = 0.0 if offsets == 'zero' else 0.02
                sd[k + 'weight'] = torch.randn((n, planes, 3, 3), generator=g) * std
                sd[k + 'bias'] = torch.randn((n,), generator=g) * (0.0 if offsets == 'zero' else 0.3)
    return hvrnet_amd.build_model(cfg, sd, dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_dcn_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(dict(modulated=True, deformable_groups=2, fallback_on_stride=False), torch.bfloat16, 'random')
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [torch.cat([S.synth_frame(10 * c + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV) for c in range(2)]
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
            n_det += sum(len(r) for r in got[-1])
    assert n_det > 0


def test_zero_offset_dcn_window_detects_what_the_plain_model_detects_in_f32():
    """DCN v1 with zero-initialised offset convs IS the plain conv: the dcn model must detect what the dcn-free model with the same
    weights detects, inside the frozen tolerance of hvrnet_amd/parity.py (f32 mode: two f32 evaluations of one function)."""
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(40 + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    plain = _eager(_window_model(None, torch.float32, None), clip, metas)
    dcn = _eager(_window_model(dict(modulated=False, deformable_groups=1, fallback_on_stride=False), torch.float32, 'zero'), clip, metas)
    assert len(plain) == len(dcn) == 2
    for got, want in zip(dcn, plain):
        st = parity.strict(got, want)
        print('zero-offset dcn vs plain (f32): %s' % st)
        assert st['n'] > 0 and parity.within_tolerance(st), st
