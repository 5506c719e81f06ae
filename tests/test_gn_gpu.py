"""GPU tests of the GroupNorm path: the two kernels (native.group_norm_stats / group_norm_apply) against the f64 statement of
tests/gn_refs.py in bf16, f16 and f32 over the geometries, operand families and variants of its table, guard rows behind y and ws, the
exact family, determinism and graph replay, the refused shapes; Bottlenecks, the stem and the golden blocks under
norm_cfg = dict(type='GN', ...) against the hand-made chain of public native calls with every norm link held to its statement in all
four modes; and a small R-50-GN + ResLayer window eager / graphed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import gn_refs as R  # noqa: E402
from tests.test_gn_refs import GN32, golden_blocks  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': SPLIT, 'f32': torch.float32}
KERNEL_MODES = ('bf16', 'f16', 'f32')
GUARD, SENTINEL = 4096, 7777


def _dev(a, mode):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DTYPES[mode]).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)


def _case(geo, family, mode, seed=0):
    B, H, W, C, G = geo
    P = H * W
    u = R.operands(family, mode, B, P, C, G, seed)
    resid = R.operands('real', mode, B, P, C, G, seed + 1)
    (gamma, beta), (gr, br) = R.affine(C, seed + 2), R.affine(C, seed + 3)
    return dict(u=u, resid=resid, gamma=gamma, beta=beta, gr=gr, br=br)


def _run(c, geo, mode, variant, relu, place='fresh'):
    """The kernels on the case -> (stored values f64 [B,P,C], raw y, guards untouched).  variant: 'plain' | 'resid' | 'normed'; place: 'fresh'
    (y in a sentinel-filled buffer with guard elements behind it) | 'u' | 'resid' (y is that input)."""
    B, H, W, C, G = geo
    u, resid = _dev(c['u'], mode).view(B, H, W, C), _dev(c['resid'], mode).view(B, H, W, C)
    ws = native.group_norm_stats(u, G)
    S_ = native.group_norm_splits(B, H * W, C)
    assert tuple(ws.shape) == (B, S_, G, 4) and S_ == R.splits(B, H * W)[0]
    rn = (native.group_norm_stats(resid, G), _f32(c['gr']), _f32(c['br'])) if variant == 'normed' else None
    n = B * H * W * C
    buf = torch.full((n + GUARD,), SENTINEL, dtype=DTYPES[mode], device=DEV)
    out = {'fresh': buf[:n].view(B, H, W, C), 'u': u, 'resid': resid}[place]
    y = native.group_norm_apply(u, ws, _f32(c['gamma']), _f32(c['beta']), R.EPS, G, None if variant == 'plain' else resid, rn, relu, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    return y.double().cpu().view(B, H * W, C).numpy(), y, bool((buf[n:] == SENTINEL).all())


def _statement(c, geo, variant, relu):
    B, H, W, C, G = geo
    return R.gn_statement(c['u'], c['gamma'], c['beta'], G, R.EPS, None if variant == 'plain' else c['resid'],
                          (c['gr'], c['br']) if variant == 'normed' else None, relu, S=R.splits(B, H * W)[0])


def _hold(got, st, mode, what):
    lo, hi = F.stored_bracket(torch.from_numpy(st['y']), torch.from_numpy(st['bound']), mode)
    g = torch.from_numpy(np.ascontiguousarray(got))
    bad = int(((g < lo) | (g > hi)).sum())
    err = float((g - torch.from_numpy(st['y'])).abs().max())
    print('%s %s: max |got - ref| = %.3g of scale %.3g, widest bound %.3g, %d of %d outside' % (what, mode, err, float(np.abs(st['y']).max()),
                                                                                           float(st['bound'].max()), bad, g.numel()))
    assert bad == 0, (what, mode, err, bad)


# ------------------------------------------------------------------------------------------------ kernel vs statement
@pytest.mark.parametrize('mode', KERNEL_MODES)
@pytest.mark.parametrize('geo', R.GEOMETRIES, ids=lambda g: 'x'.join(str(v) for v in g))
def test_kernels_against_the_statement(geo, mode):
    for family in ('real', 'offset'):
        c = _case(geo, family, mode, seed=sum(geo))
        for variant, relu, place in (('plain', False, 'fresh'), ('plain', True, 'u'), ('resid', True, 'fresh'), ('resid', False, 'resid'),
                                     ('normed', True, 'fresh'), ('normed', True, 'u'), ('normed', False, 'resid')):
            got, _, guard = _run(c, geo, mode, variant, relu, place)
            assert guard, 'guard elements behind y were written'
            _hold(got, _statement(c, geo, variant, relu), mode, '%s %s %s relu=%d y=%s' % (geo, family, variant, relu, place))
        assert float(np.abs(_statement(c, geo, 'plain', False)['y']).max()) > 0.5


@pytest.mark.parametrize('mode', KERNEL_MODES)
def test_several_runs_with_a_ragged_last_one(mode):
    B, H, W, C, G = geo = R.RAGGED
    S_, chunk = R.splits(B, H * W)
    assert native.group_norm_splits(B, H * W, C) == S_ == 64 and chunk == 265 and 0 < H * W - (S_ - 1) * chunk < chunk   # the last run holds 204 pixels
    c = _case(geo, 'real', mode, seed=5)
    c['u'][:, (S_ - 1) * chunk:] += 3.0          # the last run differs from the others: dropping it or weighing it as a full run shows
    c['u'] = _dev(c['u'], mode).double().cpu().numpy()       # (back on the format's grid)
    got, y, guard = _run(c, geo, mode, 'normed', True)
    assert guard
    st = _statement(c, geo, 'normed', True)
    _hold(got, st, mode, 'ragged %s' % (geo,))
    for mistake in ('last_run_dropped', 'run_weights_equal'):
        wrong = R.gn_statement(c['u'], c['gamma'], c['beta'], G, R.EPS, c['resid'], (c['gr'], c['br']), True, mistake=mistake, S=S_)['y']
        lo, hi = F.stored_bracket(torch.from_numpy(st['y']), torch.from_numpy(st['bound']), mode)
        w = torch.from_numpy(wrong).float().to(DTYPES[mode]).double()
        assert int(((w < lo) | (w > hi)).sum()) > 0, mistake
    # a workspace with guard elements behind it: the stats pass writes its B * S * G * 4 floats and nothing else
    u = _dev(c['u'], mode).view(B, H, W, C)
    nbytes = native.lib().hvr_gn_workspace_bytes(B, H * W, C, G)
    buf = torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    native._check(native.lib().hvr_gn_stats(native._ptr(u), native._ptr(buf), nbytes, B, H * W, C, G, native._dt(u), native._stream()), 'hvr_gn_stats')
    torch.cuda.synchronize()
    n = B * S_ * G * 4
    assert bool((buf[n:] == SENTINEL).all()) and torch.equal(buf[:n].view(B, S_, G, 4), native.group_norm_stats(u, G))
    counts = buf[:n].view(B, S_, G, 4)[0, :, 0, 0].cpu()
    assert float(counts[:-1].min()) == float(counts[:-1].max()) == chunk * (C // G) and float(counts[-1]) == 204 * (C // G)


@pytest.mark.parametrize('mode', KERNEL_MODES)
def test_constant_groups_are_exact(mode):
    for geo in ((2, 5, 7, 128, 8), (3, 19, 23, 128, 32), (1, 6, 5, 2048, 32)):
        B, H, W, C, G = geo
        c = _case(geo, 'constant', mode, seed=3)
        for variant in ('plain', 'resid'):
            got, _, guard = _run(c, geo, mode, variant, True)
            v = _f32(c['beta']).view(1, 1, C).expand(B, H * W, C)
            if variant == 'resid':
                v = v + _f32(c['resid'])
            want = torch.relu(v).to(DTYPES[mode]).double().cpu().numpy()
            assert guard and np.array_equal(got, want), (geo, mode, variant)


def test_two_calls_are_bit_equal_and_a_graph_replay_equals_eager():
    geo = B, H, W, C, G = (3, 19, 23, 128, 32)
    c = _case(geo, 'real', 'bf16', seed=9)
    u, resid = _dev(c['u'], 'bf16').view(B, H, W, C), _dev(c['resid'], 'bf16').view(B, H, W, C)
    ga, be, gr, br = _f32(c['gamma']), _f32(c['beta']), _f32(c['gr']), _f32(c['br'])

    def run():
        return native.group_norm(u, ga, be, G, R.EPS, resid=resid, resid_norm=(native.group_norm_stats(resid, G), gr, br), relu=True)
    a, b = run(), run()
    assert torch.equal(a, b) and torch.equal(native.group_norm_stats(u, G), native.group_norm_stats(u, G))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = run()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, a)


def test_refused_shapes_name_the_constraint():
    def call(C, G, dtype=torch.bfloat16):
        u = torch.zeros((1, 2, 2, C), dtype=dtype, device=DEV)
        return native.group_norm(u, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), G, 1e-5)
    for C, G, word in ((64, 64, 'Cg=1'), (2048, 16, 'Cg=128'), (96, 32, 'C=96'), (4096, 64, 'C=4096'), (256, 48, 'does not divide')):
        assert not native.group_norm_supported(C, G, torch.bfloat16)
        with pytest.raises(native.HvrError, match=word):
            call(C, G)
    assert native.group_norm_supported(64, 32, torch.bfloat16) and native.group_norm_supported(2048, 32, torch.float32)
    assert native.group_norm_supported(256, 32, SPLIT)        # (through the f32 kernels, cast by the caller)
    split = native.cast(torch.zeros((1, 2, 2, 64), device=DEV), SPLIT)
    with pytest.raises(native.HvrError, match='split-half'):
        native.group_norm_stats(split, 32)
    with pytest.raises(native.HvrError, match='split-half'):
        native._check(native.lib().hvr_gn_stats(native._ptr(split), native._ptr(split), 1 << 20, 1, 4, 64, 32, native.HVR_F16S, native._stream()), 'hvr_gn_stats')
    assert native.lib().hvr_abi_version() == 7


# ------------------------------------------------------------------------------------------------ modules
def _values(t):
    return F.values(t).double().cpu()


def _norm_link(u, affine, G, eps, mode, relu, resid=None, rn=None, keep_f32=False):
    """native.group_norm on the chain's own u (compute format; split half: f32, the result cast) with the link held to its statement."""
    um = 'f32' if mode == 'f16x2' else mode
    y = native.group_norm(u, affine[0], affine[1], G, eps, resid, rn, relu)
    B, H, W, C = u.shape
    np_ = lambda t: t.double().cpu().view(B, H * W, C).numpy()   # noqa: E731
    st = R.gn_statement(np_(u), affine[0].double().cpu().numpy(), affine[1].double().cpu().numpy(), G, eps, None if resid is None else np_(resid),
                        None if rn is None else (rn[1].double().cpu().numpy(), rn[2].double().cpu().numpy()), relu, S=R.splits(B, H * W)[0])
    _hold(np_(y), st, um, 'link %s G=%d' % (tuple(u.shape), G))
    return native.cast(y, SPLIT) if mode == 'f16x2' and not keep_f32 else y


def _hand_block(blk, x, mode):
    """The block as a chain of public native calls on its packed weights."""
    p, split = blk.packed(x.device), mode == 'f16x2'
    G, Gw, eps = blk.num_groups, blk.gn_width_groups, blk.gn_eps
    conv = lambda t, w, **kw: native.conv2d_nhwc(t, w, None, relu=False, out_f32=split, **kw)   # noqa: E731
    h = _norm_link(conv(x, p['c1'], stride=blk.conv1_stride), p['n1'], Gw, eps, mode, True)
    h = _norm_link(conv(h, p['c2'], stride=blk.conv2_stride, pad=blk.dilation, dil=blk.dilation), p['n2'], Gw, eps, mode, True)
    u = conv(h, p['c3'])
    if blk.downsample is not None:
        resid = conv(x, p['ds'], stride=blk.stride)
        rn = (native.group_norm_stats(resid, G),) + p['nd']
    else:
        resid, rn = native.cast(x, torch.float32) if split else x, None
    return _norm_link(u, p['n3'], G, eps, mode, True, resid, rn)


def _block(inplanes, planes, stride=1, dilation=1, style='pytorch', proj=False, seed=0):
    cfg = GN32
    down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), torch.nn.GroupNorm(32, 4 * planes)) if proj else None
    blk = backbone.Bottleneck(inplanes, planes, stride, dilation, down, style=style, norm_cfg=cfg)
    g = torch.Generator().manual_seed(seed)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) / (m.weight[0].numel()) ** 0.5
        elif isinstance(m, torch.nn.GroupNorm):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
    return blk


BLOCKS = dict(identity=(lambda: _block(256, 64), (2, 10, 12, 256)),
              stride2=(lambda: _block(256, 128, stride=2, proj=True, seed=1), (2, 10, 12, 256)),
              caffe=(lambda: _block(512, 128, stride=2, style='caffe', proj=True, seed=2), (2, 10, 12, 512)),
              res5=(lambda: _block(1024, 512, dilation=2, proj=True, seed=3), (1, 6, 8, 1024)),
              golden=(lambda: golden_blocks()[1]['a'], (2, 9, 11, 128)))


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('name', sorted(BLOCKS))
def test_gn_bottleneck_is_the_chain_of_native_calls(name, mode):
    make, shape = BLOCKS[name]
    blk = make().to(DEV).eval()
    backbone.set_compute_dtype(blk, DTYPES[mode])
    x = native.cast(torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(DEV), DTYPES[mode])
    step = blk.plan_close(shape[0], shape[1], shape[2], DTYPES[mode])
    assert step.kind == 'gn' and step.downsample == (blk.downsample is not None)
    with torch.no_grad():
        y = blk.forward_nhwc(x)
        want = _hand_block(blk, x, mode)
    assert y.dtype == DTYPES[mode] and torch.equal(y, want)
    v = _values(y)
    assert float(v.abs().max()) > 0.1 and float(v.min()) >= 0.0
    if name == 'golden':      # the channels that pad conv1 / conv2 to 64 hold exact zeros
        p = blk.packed(x.device)
        h = native.group_norm(native.conv2d_nhwc(x, p['c1'], None, out_f32=mode == 'f16x2'), p['n1'][0], p['n1'][1], blk.gn_width_groups, blk.gn_eps,
                              relu=True)
        assert h.shape[-1] == 64 and float(h[..., 32:].float().abs().max()) == 0.0 and float(h[..., :32].float().abs().max()) > 0


@pytest.mark.parametrize('mode', F.MODES)
def test_gn_stem_is_its_chain(mode):
    net = hvrnet_amd.ResNet(depth=50, num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,), norm_cfg=GN32)
    sd = S.synth_state_dict(depth=50, norm='GN')
    net.load_state_dict({k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.') and not k.startswith(('backbone.layer2', 'backbone.layer3'))},
                        strict=True)
    net = net.to(DEV).eval()
    backbone.set_compute_dtype(net, DTYPES[mode])
    x = torch.randn((2, 3, 64, 80), generator=torch.Generator().manual_seed(11)).to(DEV)
    with torch.no_grad():
        p = net.packed(x.device)
        y = net._stem(x, p)
        cols, OH, OW = native.im2col_stem(x.contiguous().float(), DTYPES[mode], backbone.STEM_KP)
        u = native.gemm(cols, p['stem'][0], None, relu=False, out_f32=mode == 'f16x2').view(2, OH, OW, 64)
        h = _norm_link(u, p['gn'], 32, net.gn_eps, mode, True, keep_f32=True)      # (split half is pooled in f32, then cast)
        want = native.cast(native.maxpool3x3s2_nhwc(h), DTYPES[mode])
    assert tuple(y.shape) == (2, 16, 20, 64) and y.dtype == DTYPES[mode] and torch.equal(y, want) and float(_values(y).abs().max()) > 0.1


def test_golden_blocks_on_the_device_in_f32():
    """The reference's two f64 blocks under GroupNorm (tests/golden/g25_gn_block.npz) through this project's Bottleneck in f32 mode.  The
    bound, from the formats alone: a conv link errs by at most (K + 3) u sum|x||w| with K <= 288 and u = 2^-24, the f32 rounding of the
    parameters adds u per factor, and sum|x||w| of a link is some tens of its output's spread; the norm behind it divides by that spread, so
    a link hands on at most 291 x 6e-8 x 40 = 7e-4 of a unit-scale map times gamma <= 1.5, plus the norm's own (tests/gn_refs.py: a few
    1e-6).  Three links in a row, the first two damped by the next conv's averaging no further than 1: 3 x 1.05e-3 = 3.2e-3 -> 4e-3 of
    the output's largest value (8.3 and 7.5).  A wrong group map or variance errs by the output's own scale."""
    z, blocks = golden_blocks()
    for name, blk in blocks.items():
        blk = blk.to(DEV).eval()
        backbone.set_compute_dtype(blk, torch.float32)
        with torch.no_grad():
            y = blk(torch.from_numpy(z['x']).float().to(DEV))
        want = torch.from_numpy(z[name + '.out'])
        assert tuple(y.shape) == tuple(want.shape)
        err = float((y.double().cpu() - want).abs().max())
        print('golden GN block %s in f32: max |y - ref| = %.3g of scale %.3g' % (name, err, float(want.abs().max())))
        assert err <= 4e-3 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ an R-50-GN window
HW, PAD = (120, 150), (128, 160)
T, NPROP = 3, 16


def _window_model(dtype):
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(type='ResNet', depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='pytorch',
                              norm_cfg=dict(type='GN', num_groups=32, requires_grad=False), norm_eval=True)
    cfg.model.shared_head = dict(type='ResLayer', depth=50, stage=3, stride=1, dilation=2, style='pytorch', norm_cfg=dict(type='GN', num_groups=32),
                                 norm_eval=True, external_conv=True)
    return hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', depth=50, norm='GN'), dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_gn_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert model.backbone.with_gn and model.shared_head.with_gn and isinstance(model.backbone.gn1, torch.nn.GroupNorm)
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
