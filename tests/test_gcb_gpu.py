"""GPU tests of the global context block: the three kernels (native.gcb_pool / gcb_transform / gcb_apply, native.context_block) against
the f64 statement of tests/gcb_refs.py in all four compute modes with its bounds, the overflow family, the exact cases, the aliased
apply, the refused shapes, Bottlenecks with a context block against the hand-made chain of public native calls, the reference's golden
blocks in f32, and a small window with context blocks in layers 2 and 3, eager and graphed."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import gcb_refs as R  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': native.SPLIT, 'f32': torch.float32}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_gcb_block.npz')
FUSIONS = (('channel_add', ), ('channel_mul', ), ('channel_add', 'channel_mul'))


def _dev(x, shape, mode):
    """Stored-format f64 values [B,P,C] -> the device map [B,H,W,C] of `mode`."""
    if x is None:
        return None
    return D.to_device_operand(torch.from_numpy(x).reshape(shape), mode, DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().contiguous().to(DEV)


def _packed(prm):
    def branch(br):
        if br is None:
            return None
        w1, b1, gamma, beta, w2, b2 = br
        return (_f32(w1), _f32(b1), _f32(gamma), _f32(beta), _f32(w2.T), _f32(b2))
    return dict(wm=_f32(prm['wm']) if prm.get('wm') is not None else None, mul=branch(prm.get('mul')), add=branch(prm.get('add')))


def _vals(t):
    v = F.values(t).cpu().numpy()
    return v.reshape(v.shape[0], -1, v.shape[-1])


def _hold(c, mode, relu, what):
    """The whole block on the device against the statement; in the native modes m and t against their own bounds as well."""
    shape, prm = c['shape'], c['prm']
    r = R.context_statement(c['u'], prm, c['resid'], relu)
    u, resid, pk = _dev(c['u'], shape, mode), _dev(c['resid'], shape, mode), _packed(prm)
    y = native.context_block(u, pk, resid, relu)
    assert y.dtype == DTYPES[mode] and tuple(y.shape) == tuple(shape)
    bound = R.context_bound(c['u'], prm, c['resid'], mode, r)
    got = _vals(y)
    err = np.abs(got - r['y'])
    print('%s %s %s: worst |y - ref| / bound = %.3f (max bound %.3g)' % (what, shape, mode, float((err / bound).max()), float(bound.max())))
    assert np.abs(r['y']).max() > 0.5
    assert R.outside(got, r['y'], bound) == 0, (what, shape, mode, float((err / bound).max()))
    # link by link (f32 kernels serve split half: its links run on the f32 form, and the block equals their chain bit for bit)
    B, H, W, C = shape
    lm = 'f32' if mode == 'f16x2' else mode
    if mode == 'f16x2':
        u, resid = native.cast(u, torch.float32), None if resid is None else native.cast(resid, torch.float32)
    part = native.gcb_pool(u, pk['wm'])
    assert tuple(part.shape) == (B, R.splits(B, H * W)[0], C + 4) and native.gcb_splits(B, H * W, C) == R.splits(B, H * W)[0]
    pnp = part.double().cpu().numpy()
    ctx_dev, _ = R.combine(pnp)
    dctx = R.pool_bound(c['u'], prm.get('wm'), r)
    print('    ctx: worst / bound = %.3f (bound / |ctx| max %.2g)' % (float((np.abs(ctx_dev - r['ctx']) / dctx).max()), float((dctx / np.abs(r['ctx']).max()).max())))
    assert R.outside(ctx_dev, r['ctx'], dctx) == 0, (what, 'ctx')
    m, t = native.gcb_transform(part, H * W, pk['mul'], pk['add'])
    rm, rt = R.transform_statement(ctx_dev, prm.get('mul'), prm.get('add'))
    dm, dt = R.transform_bound(ctx_dev, R.combine_bound(pnp), prm.get('mul'), prm.get('add'))
    for g_, ref, b, name in ((m, rm, dm, 'm'), (t, rt, dt, 't')):
        assert (g_ is None) == (ref is None)
        if g_ is not None:
            e = np.abs(g_.double().cpu().numpy() - ref)
            print('    %s: worst / bound = %.3f (max bound %.2g)' % (name, float((e / b).max()), float(b.max())))
            assert R.outside(g_.double().cpu().numpy(), ref, b) == 0, (what, name, float((e / b).max()))
    y2 = native.gcb_apply(u, m, t, resid, relu)
    md, td = (None if m is None else m.double().cpu().numpy()), (None if t is None else t.double().cpu().numpy())
    ry = R.apply_statement(c['u'], md, td, c['resid'], relu)
    assert R.outside(_vals(y2), ry, R.apply_bound(c['u'], md, td, c['resid'], None, None, lm, ry)) == 0, (what, 'apply')
    assert torch.equal(native.cast(y2, DTYPES[mode]), y) if mode == 'f16x2' else torch.equal(y2, y)
    return r, got, bound


# ------------------------------------------------------------------------------------------------ kernels vs statement
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('shape', R.SHAPES)
def test_block_against_statement(mode, shape):
    """'att' and 'avg' x {add, mul, both}, the bottleneck widths 4 / 16 / 76 in turn, with and without the residual and the ReLU."""
    i = 0
    for pooling in ('att', 'avg'):
        for fusion in FUSIONS:
            c = R.real_case(shape, mode, 500 + 7 * i + shape[3], pooling, fusion, R.PLANES[i % 3], with_resid=i % 2 == 0)
            _hold(c, mode, relu=i % 2 == 0, what='%s %s R=%d' % (pooling, '+'.join(f[8:] for f in fusion), R.PLANES[i % 3]))
            i += 1


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('peak', ('first', 'last'))
def test_overflow_family(mode, peak):
    """Logits over about +-100 with the frame maximum in the first / the last run and a run whose weights underflow to exactly 0: the
    output is finite and inside the bound.  A kernel that does not subtract the running maximum cannot pass: exp(100) is inf in f32
    (asserted on the inputs), and the statement with that mistake is not even finite."""
    c = R.overflow_case(R.SHAPES[2], mode, 77, peak)
    l = R.pool_statement(c['u'], c['prm']['wm'])['l']
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(np.float32(l.max())))
    assert float(np.exp(np.float32(l[:, c['lo']].max() - l.max()))) == 0.0
    r, got, bound = _hold(c, mode, True, 'overflow peak %s' % peak)
    assert np.isfinite(got).all()
    bad = R.context_statement(c['u'], c['prm'], c['resid'], True, 'no_max')['y']
    assert R.outside(bad, r['y'], bound) > 0


# ------------------------------------------------------------------------------------------------ exact cases
def test_zero_mask_weights_give_the_mean():
    """wm = 0: every logit is 0, every weight 1 -- the attention pool IS the average pool, bit for bit, and both lie at the mean."""
    for shape in R.SHAPES:
        c = R.real_case(shape, 'f32', 31, 'avg', FUSIONS[2], 16)
        u, pk = _dev(c['u'], shape, 'f32'), _packed(c['prm'])
        P = shape[1] * shape[2]
        pa = native.gcb_pool(u, torch.zeros(shape[3], dtype=torch.float32, device=DEV)).clone()
        pv = native.gcb_pool(u, None).clone()
        assert torch.equal(pa, pv)
        ctx = (pv[:, :, 4:] * 1.0).sum(1) / pv[:, :, 1].sum(1, keepdim=True)
        mean = c['u'].mean(1)
        assert np.abs(ctx.double().cpu().numpy() - mean).max() <= (P + 16) * R.U32 * np.abs(c['u']).mean(1).max()
        assert float(pv[:, :, 1].sum()) == shape[0] * P and float(pv[:, :, 0].abs().max()) == 0.0


@pytest.mark.parametrize('mode', R.MODES)
def test_zero_last_conv_is_the_plain_close(mode):
    """channel_add with a zero last conv (the reference's initial state): y == relu(u + identity), bit for bit."""
    shape = R.SHAPES[2]
    c = R.real_case(shape, mode, 32, 'att', FUSIONS[0], 16)
    w1, b1, gamma, beta, w2, b2 = c['prm']['add']
    c['prm']['add'] = (w1, b1, gamma, beta, np.zeros_like(w2), np.zeros_like(b2))
    u, resid = _dev(c['u'], shape, mode), _dev(c['resid'], shape, mode)
    y = native.context_block(u, _packed(c['prm']), resid, True)
    want = torch.relu(native.cast(u, torch.float32) + native.cast(resid, torch.float32))
    assert torch.equal(native.cast(y, torch.float32), native.cast(native.cast(want, DTYPES[mode]), torch.float32))


def test_one_hot_softmax_selects_the_pixel():
    """One pixel's logit 80 above the rest (wm = e_0, channel 0 carries the logit): its weight is 1 and the others' contributions vanish
    below half an ulp, so the run that holds it has sum == 1 and acc == u[p*] exactly, and m, t equal those of the one-pixel map u[p*]."""
    shape = R.SHAPES[2]
    B, H, W, C = shape
    P = H * W
    S, chunk = R.splits(B, P)
    c = R.real_case(shape, 'f32', 33, 'att', FUSIONS[2], 16)
    star = [5, chunk * 7 + 11, P - 1]                      # in the first run, in a middle run, the last pixel of the ragged last run
    c['u'][:, :, 0] *= 0.25
    for b in range(B):
        c['u'][b, star[b], 0] = 82.0
    c['u'] = R.stored(c['u'], 'f32')
    wm = np.zeros(C)
    wm[0] = 1.0
    c['prm']['wm'] = wm
    u, pk = _dev(c['u'], shape, 'f32'), _packed(c['prm'])
    part = native.gcb_pool(u, pk['wm']).clone()
    m, t = native.gcb_transform(part, P, pk['mul'], pk['add'])
    one = torch.stack([u.view(B, P, C)[b, star[b]] for b in range(B)]).view(B, 1, 1, C).contiguous()
    m1, t1 = native.gcb_transform(native.gcb_pool(one, pk['wm']), 1, pk['mul'], pk['add'])
    for b in range(B):
        slab = part[b, star[b] // chunk]
        assert float(slab[0]) == 82.0 and float(slab[1]) == 1.0 and torch.equal(slab[4:], one[b, 0, 0])
    assert torch.equal(m, m1) and torch.equal(t, t1)


@pytest.mark.parametrize('mode', ('bf16', 'f16', 'f32'))
def test_apply_in_place(mode):
    shape = R.SHAPES[2]
    c = R.real_case(shape, mode, 34)
    u, resid = _dev(c['u'], shape, mode), _dev(c['resid'], shape, mode)
    m = torch.rand((shape[0], shape[3]), device=DEV)
    t = torch.randn((shape[0], shape[3]), device=DEV)
    want = native.gcb_apply(u, m, t, resid, True)
    ref = R.apply_statement(c['u'], m.double().cpu().numpy(), t.double().cpu().numpy(), c['resid'], True)
    assert R.outside(_vals(want), ref, R.apply_bound(c['u'], m.double().cpu().numpy(), t.double().cpu().numpy(), c['resid'], None, None, mode, ref)) == 0
    u2 = u.clone()
    got = native.gcb_apply(u2, m, t, resid, True, out=u2)
    assert got.data_ptr() == u2.data_ptr() and torch.equal(got, want)
    assert torch.equal(native.gcb_apply(u, None, t, None, False), (u.float() + t[:, None, None, :]).to(u.dtype))


def test_refused_shapes():
    x = torch.zeros((2, 5, 7, 96), dtype=torch.bfloat16, device=DEV)
    assert not native.gcb_supported(96, torch.bfloat16) and native.gcb_supported(2048, native.SPLIT) and not native.gcb_supported(2112, torch.float32)
    with pytest.raises(native.HvrError):
        native.gcb_pool(x)
    ok = torch.zeros((2, 5, 7, 128), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(native.HvrError):
        native.gcb_pool(ok[:, :, ::2])                     # not contiguous
    with pytest.raises(native.HvrError):
        native.gcb_pool(ok, torch.zeros(128, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(native.HvrError):
        native.gcb_pool(ok.to(torch.int64))
    with pytest.raises(native.HvrError):
        native.gcb_apply(ok, torch.zeros((2, 128), dtype=torch.bfloat16, device=DEV))
    with pytest.raises(native.HvrError):
        native.gcb_apply(ok, None, torch.zeros((2, 128), device=DEV), resid=ok.float())
    with pytest.raises(native.HvrError):
        native.gcb_apply(ok, None, torch.zeros((3, 128), device=DEV))
    with pytest.raises(native.HvrError):
        native.gcb_transform(native.gcb_pool(ok), 35)      # neither branch
    with pytest.raises(native.HvrError):
        native.context_block(x, dict(wm=None, mul=None, add=None))
    with pytest.raises(NotImplementedError):
        ops.ContextBlock(128, 0.25)(torch.zeros((1, 128, 4, 4)))


# ------------------------------------------------------------------------------------------------ Bottlenecks
def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g) / fan ** 0.5
            if m.bias is not None:
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
        elif isinstance(m, torch.nn.BatchNorm2d):
            n = m.weight.shape[0]
            m.weight.data, m.bias.data = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.2
            m.running_mean.data, m.running_var.data = torch.randn(n, generator=g) * 0.2, torch.rand(n, generator=g) + 0.5
        elif isinstance(m, torch.nn.LayerNorm):
            m.weight.data, m.bias.data = torch.rand(m.weight.shape, generator=g) + 0.5, torch.randn(m.bias.shape, generator=g) * 0.2
    return module


def _hand_made(blk, x):
    p, s = blk.packed(x.device), blk.stride
    h = native.conv2d_nhwc(x, p['c1'][0], p['c1'][1], relu=True, stride=blk.conv1_stride)
    h = native.conv2d_nhwc(h, p['c2'][0], p['c2'][1], relu=True, stride=blk.conv2_stride, pad=blk.dilation, dil=blk.dilation)
    u = native.conv2d_nhwc(h, p['c3'][0], p['c3'][1], relu=False)
    identity = native.conv2d_nhwc(x, p['ds'][0], p['ds'][1], relu=False, stride=s) if blk.downsample is not None else x
    return native.context_block(u, blk.context_block.packed(x.device), resid=identity, relu=True)


@pytest.mark.parametrize('mode', R.MODES)
def test_bottleneck_and_chain_equal_the_hand_made_chain(mode):
    gcb = dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))
    layer = _randomise(backbone.make_res_layer(backbone.Bottleneck, 128, 64, 2, stride=2, style='caffe', gcb=gcb), 41).to(DEV).eval()
    backbone.set_compute_dtype(layer, DTYPES[mode])
    assert all(b.with_gcb and b.context_block.planes == 64 for b in layer)
    x = D.to_device_operand(torch.randn((2, 13, 17, 128), generator=torch.Generator().manual_seed(42)).double(), mode, DEV)
    with torch.no_grad():
        y0 = layer[0].forward_nhwc(x)
        assert str(layer[0].plan_close(2, 13, 17, DTYPES[mode], layer[1])) == 'downsample+gcb' and tuple(y0.shape) == (2, 7, 9, 256)
        w0 = _hand_made(layer[0], x)
        assert torch.equal(y0, w0)
        y1, w1 = layer[1].forward_nhwc(y0), _hand_made(layer[1], w0)
        assert torch.equal(y1, w1) and float(F.values(y1).abs().max()) > 0.5
        # the block is not the plain Bottleneck: without the context block the output differs
        plain = native.conv2d_nhwc(layer[1].body(y0), *layer[1].packed(x.device)['c3'], resid=y0, relu=True)
        assert not torch.equal(plain, y1)


def _golden_sd(z, name):
    return {k[len(name) + 1:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith(name + '.') and k.split('.')[-1] not in ('x', 'out', 'out_f32')}


def test_golden_blocks_on_the_device_in_f32():
    """The reference's two stand-alone context blocks and two Bottlenecks with one (tests/golden/g23_gcb_block.npz) through this project's
    modules in f32 mode, within gcb_refs.block_bound_f32 (derivation there)."""
    z = np.load(GOLDEN)
    down = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, stride=2, bias=False), torch.nn.BatchNorm2d(128))
    mods = dict(ca=ops.ContextBlock(128, 1. / 8., 'att', ('channel_add', 'channel_mul')), cb=ops.ContextBlock(64, 0.31, 'avg', ('channel_mul', )),
                pa=backbone.Bottleneck(64, 32, stride=2, downsample=down, gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))),
                pb=backbone.Bottleneck(128, 32, gcb=dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', ))))
    for name, mod in mods.items():
        mod.load_state_dict(_golden_sd(z, name), strict=True)
        mod = mod.to(DEV).eval()
        backbone.set_compute_dtype(mod, torch.float32)
        with torch.no_grad():
            y = mod(torch.from_numpy(z[name + '.x']).float().to(DEV))
        want = torch.from_numpy(z[name + '.out'])
        assert tuple(y.shape) == tuple(want.shape)
        err = float((y.double().cpu() - want).abs().max())
        print('golden %s in f32: max |y - ref| = %.3g of scale %.3g' % (name, err, float(want.abs().max())))
        assert err <= R.block_bound_f32(float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ a window with context blocks
HW, PAD = (120, 150), (128, 160)
T, NPROP = 3, 16
GCB = dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))


def _window_model(dtype):
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(cfg.model.backbone, depth=50, gcb=GCB, stage_with_gcb=(False, True, True))
    cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
    return hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', depth=50, gcb=GCB), dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_gcb_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    bb = model.backbone
    assert [any(b.with_gcb for b in getattr(bb, n)) for n in bb.res_layers] == [False, True, True]
    assert 'gcb' in str(bb.stage_route(1, T, 32, 40, torch.bfloat16)) and not bb.stage_route(1, T, 32, 40, torch.bfloat16).compact
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
            for dets in got[-1]:
                a = np.asarray(dets)
                assert a.ndim == 2 and a.shape[1] == 5 and np.isfinite(a).all()
                assert (a[:, 4] >= 0).all() and (a[:, 4] <= 1).all() and (a[:, 2] - a[:, 0] >= -1).all() and (a[:, 3] - a[:, 1] >= -1).all()
                assert (a[:, :4] >= 0).all() and (a[:, [0, 2]] <= HW[1]).all() and (a[:, [1, 3]] <= HW[0]).all()
                n_det += len(a)
    assert n_det > 0
