"""GPU tests of the Guided Anchoring RPN: the masked conv, the mask + offset kernel and the guided proposal entry against the f64
statements of tests/ga_rpn_refs.py with their bounds, GARPNHead end to end in all four compute modes (its forward equal to the
hand-made chain of public native calls, every link of that chain held to its statement on the stored values of the link before; its
proposals equal to the statement's read-out of the device's own maps), and a small SelsaRCNN window with a GARPNHead, eager and graphed.
hvr_ga_rpn_proposals has ONE form (no chip-wide variant, no frame-count switch): T = 2 and T = 5 run the same kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import selsa_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import ga_rpn_refs as R  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': native.SPLIT, 'f32': torch.float32}
SENTINEL = 7777.0
MAPS = ((5, 7), (9, 11))
MASKS = ('all', 'none', 'one', 'checker', 'per_frame')


def _masks(kind, B, H, W, g):
    k = np.zeros((B, H, W), bool)
    if kind == 'all':
        k[:] = True
    elif kind == 'one':
        k[B - 1, H - 1, W - 2] = True
    elif kind == 'checker':
        k[:] = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)[None]
    elif kind == 'per_frame':
        k = g.random((B, H, W)) < np.array([0.2, 0.5, 0.8] * B)[:B, None, None]
        assert not np.array_equal(k[0], k[1])
    return k


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().contiguous().to(DEV)


def _inside(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print('%s: worst |got - ref| / bound = %.3f' % (what, worst))
    assert np.isfinite(np.asarray(got)).all() and (err <= bound).all(), (what, worst)


# ------------------------------------------------------------------------------------------------ masked conv
@pytest.mark.parametrize('mode', ('bf16', 'f16', 'f32'))
@pytest.mark.parametrize('ks', (1, 3))
@pytest.mark.parametrize('cout', (1, 5, 8))
@pytest.mark.parametrize('cin', (64, 192))
@pytest.mark.parametrize('hw', MAPS)
def test_masked_conv_against_statement(hw, cin, cout, ks, mode):
    B, (H, W), pad, ldo = 3, hw, (ks - 1) // 2, cout + 3
    g = np.random.default_rng(1000 + 7 * cin + 3 * cout + ks + H)
    tg = torch.Generator().manual_seed(int(g.integers(1 << 30)))
    x = F.store_true(torch.randn((B, H, W, cin), generator=tg), mode, 'act')
    w = F.store_true(torch.randn((cout, ks, ks, cin), generator=tg) / np.sqrt(ks * ks * cin), mode, 'weight')
    bias = (torch.randn(cout, generator=tg) * 0.5).float()
    xd, wd, bd = x.to(DTYPES[mode]).to(DEV).contiguous(), w.to(DTYPES[mode]).to(DEV).contiguous(), bias.to(DEV)
    for kind in MASKS:
        keep = _masks(kind, B, H, W, g)
        ref, bound = R.masked_conv_statement(x.numpy(), w.numpy(), bias.double().numpy(), keep, pad)
        out = torch.full((B, H, W, ldo), SENTINEL, device=DEV)
        got = native.masked_conv2d_nhwc(xd, wd, bd, torch.from_numpy(keep.astype(np.uint8)).to(DEV), pad=pad, out=out)
        assert got.data_ptr() == out.data_ptr()
        o = out.cpu()
        assert bool((o[..., cout:] == SENTINEL).all()), 'padding columns of the output pitch were written'
        o = o[..., :cout].numpy()
        assert (o[~keep].view(np.uint32) == 0).all(), 'an unkept pixel is not +0 in every channel (%s)' % kind
        if keep.any():
            assert kind != 'all' or float(np.abs(ref[keep]).max()) > 0.2
            _inside(o[keep], ref[keep], bound[keep], 'masked conv %s %dx%d cin %d cout %d k%d %s' % (mode, H, W, cin, cout, ks, kind))
    fresh = native.masked_conv2d_nhwc(xd, wd, None, torch.ones((B, H, W), dtype=torch.uint8, device=DEV), pad=pad)     # no bias, fresh output
    ref, bound = R.masked_conv_statement(x.numpy(), w.numpy(), None, np.ones((B, H, W), bool), pad)
    assert tuple(fresh.shape) == (B, H, W, cout)
    _inside(fresh.cpu().numpy(), ref, bound, 'no bias')


def test_masked_conv_refusals():
    x = torch.zeros((1, 5, 7, 64), dtype=torch.bfloat16, device=DEV)
    keep = torch.ones((1, 5, 7), dtype=torch.uint8, device=DEV)
    assert native.masked_conv_max_cout() >= 8
    w = torch.zeros((native.masked_conv_max_cout() + 1, 1, 1, 64), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(native.HvrError, match=r'\(-2\).*Cout'):                      # HVR_EUNSUPPORTED
        native.masked_conv2d_nhwc(x, w, None, keep)
    xs = native.cast(torch.zeros((1, 5, 7, 64), device=DEV), native.SPLIT)
    ws = native.cast(torch.zeros((5, 1, 1, 64), device=DEV), native.SPLIT)
    with pytest.raises(native.HvrError, match=r'\(-2\).*split'):
        native.masked_conv2d_nhwc(xs, ws, None, keep)
    with pytest.raises(native.HvrError, match=r'\(-1\)'):                            # even kernel: HVR_EINVAL
        native.masked_conv2d_nhwc(x, torch.zeros((5, 2, 2, 64), dtype=torch.bfloat16, device=DEV), None, keep, pad=0)
    with pytest.raises(native.HvrError, match=r'\(-1\)'):                            # a 3x3 that is not padded to the input size
        native.masked_conv2d_nhwc(x, torch.zeros((5, 3, 3, 64), dtype=torch.bfloat16, device=DEV), None, keep, pad=0)


@pytest.mark.parametrize('cout', (5, 16))
def test_ops_masked_conv2d_nchw_form(cout):
    """ops.MaskedConv2d / ops.masked_conv2d with the reference's NCHW arguments: 5 outputs take the skinny kernel, 16 the dense conv with
    the unkept pixels zeroed; mask=None is the plain conv."""
    B, C, H, W = 3, 64, 9, 11
    tg = torch.Generator().manual_seed(40 + cout)
    m = ops.MaskedConv2d(C, cout, 3, padding=1).to(DEV)
    with torch.no_grad():
        m.weight.copy_(F.store_true(torch.randn(m.weight.shape, generator=tg) / 24.0, 'bf16', 'weight').float())
        m.bias.copy_(torch.randn(cout, generator=tg) * 0.5)
    x = F.store_true(torch.randn((B, C, H, W), generator=tg), 'bf16', 'act')
    g = np.random.default_rng(cout)
    keep = _masks('per_frame', B, H, W, g)
    xd = x.to(torch.bfloat16).to(DEV)
    wn = m.weight.detach().cpu().double().permute(0, 2, 3, 1).numpy()
    ref, bound = R.masked_conv_statement(x.permute(0, 2, 3, 1).numpy(), wn, m.bias.detach().cpu().double().numpy(), keep, 1)
    if cout > native.masked_conv_max_cout():      # the dense route: the tile engine's bound (bf16 operands, K = 576)
        _, mag, absxw = F.conv_statement(x.permute(0, 2, 3, 1), torch.from_numpy(wn), m.bias.detach().cpu().double(), pad=1, mode='bf16')
        bound = np.where(keep[..., None], F.mfma_bound(mag, absxw, 9 * C, 'bf16').numpy(), 0.0)
    with torch.no_grad():
        y = m(xd, torch.from_numpy(keep.astype(np.uint8)).to(DEV))
        yf = ops.masked_conv2d(xd, torch.from_numpy(keep.astype(np.uint8)).to(DEV), m.weight, m.bias, padding=1)
        plain = m(xd)
    assert tuple(y.shape) == (B, cout, H, W) and y.dtype == torch.float32 and torch.equal(y, yf)
    o = y.permute(0, 2, 3, 1).cpu().numpy()
    assert (o[~keep] == 0).all()
    _inside(o[keep], ref[keep], bound[keep], 'MaskedConv2d cout %d' % cout)
    xi = xd.clone()
    xi[0, :, 0:2, :] = float('inf')                                 # an overflowing map: the unkept pixels are still exactly 0
    with torch.no_grad():
        yi = m(xi, torch.from_numpy(keep.astype(np.uint8)).to(DEV)).permute(0, 2, 3, 1).cpu().numpy()
    assert (yi[~keep].view(np.uint32) == 0).all() and not np.isfinite(yi[keep]).all()
    full, mag, absxw = F.conv_statement(x.permute(0, 2, 3, 1), torch.from_numpy(wn), m.bias.detach().cpu().double(), pad=1, mode='bf16')
    _inside(plain.permute(0, 2, 3, 1).cpu().numpy(), full.numpy(), F.mfma_bound(mag, absxw, 9 * C, 'bf16').numpy(), 'mask=None')
    with pytest.raises(NotImplementedError):
        m.cpu()(x.float(), torch.from_numpy(keep.astype(np.uint8)))


# ------------------------------------------------------------------------------------------------ mask + offsets
@pytest.mark.parametrize('hw', MAPS)
def test_mask_and_offsets_against_statement(hw):
    T, (H, W), dg, thr = 3, hw, 4, 0.3
    tg = torch.Generator().manual_seed(50 + H)
    ls = torch.randn((T, H, W, 4), generator=tg) * 2.0                  # loc | shape x 2 | pad: slices of ONE conv output
    ls[..., 0] += float(np.log(thr / (1 - thr)))
    w = torch.randn((dg * 18, 2), generator=tg) * 0.3
    keep_ref, amb = R.loc_mask_statement(ls[..., 0].numpy(), thr)
    assert not amb.any() and 0 < keep_ref.mean() < 1
    om_ref, om_bound = R.offsets_statement(ls[..., 1:3].numpy(), w.numpy())
    lsd, wd = ls.to(DEV), w.to(DEV)
    ldo = dg * 18 + 3
    om = torch.full((T, H, W, ldo), SENTINEL, device=DEV)
    keep, om2 = native.ga_mask_offsets(loc=lsd[..., 0:1], loc_filter_thr=thr, shape=lsd[..., 1:3], w_off=wd, ldo=ldo, om=om)
    assert om2.data_ptr() == om.data_ptr() and keep.dtype == torch.uint8
    assert np.array_equal(keep.cpu().numpy().astype(bool), keep_ref), 'mask'
    assert bool((om[..., dg * 18:] == SENTINEL).all())
    _inside(om[..., :dg * 18].cpu().numpy(), om_ref, om_bound, 'offsets %dx%d' % (H, W))
    assert torch.equal(native.ga_loc_mask(lsd[..., 0:1], thr), keep)
    assert torch.equal(native.ga_offsets(lsd[..., 1:3], wd), om[..., :dg * 18].contiguous())
    # the pitched om goes straight into the sampler
    x = F.store_true(torch.randn((T, H, W, 64), generator=tg).clamp(min=0), 'bf16', 'act')
    om[..., dg * 18:] = 1000.0
    col = native.deform_im2col(x.to(torch.bfloat16).to(DEV), om, 3, 3, 1, 1, 1, dg, False)
    ref, bound = D.sampler_statement(x, om.cpu(), 3, 3, 1, 1, 1, dg, False)
    lo, hi = D.stored_bracket(ref, bound, 'bf16')
    assert F.compare(F.values(col).cpu(), lo, hi, ref)[1] == 0
    # the equality case of >=: sigmoid(0) == 0.5 exactly
    z = torch.tensor([0.0, -0.0, 1e-3, -1e-3], device=DEV).view(1, 1, 4, 1)
    assert native.ga_loc_mask(z, 0.5).view(-1).tolist() == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ guided proposals on prescribed maps
KW = dict(anchoring_means=(0.1, -0.05, 0.02, 0.03), anchoring_stds=(0.07, 0.07, 0.14, 0.14), target_means=(0.0, 0.0, 0.0, 0.0),
          target_stds=(0.07, 0.07, 0.11, 0.11))
CFGS = (dict(nms_pre=12, nms_post=10, max_num=9, nms_thr=0.7), dict(nms_pre=0, nms_post=6, max_num=4, nms_thr=0.5),
        dict(nms_pre=2000, nms_post=300, max_num=300, nms_thr=0.7))


def _prescribed(T, H, W, seed, thr):
    tg = torch.Generator().manual_seed(seed)
    buf = torch.randn((T, H, W, 8), generator=tg) * torch.tensor([2.0, 3.0, 3.0, 3.0, 3.0, 0, 0, 0])     # cls | reg x 4 | pad
    shape = torch.randn((T, H, W, 2), generator=tg) * 4.0
    loc = torch.randn((T, H, W, 1), generator=tg) * 2.0 + float(np.log(thr / (1 - thr)))
    shape[:, 0, 0, 0], shape[:, 1, 2, 1], shape[:, 2, 3, 0] = 120.0, -110.0, 99.0    # x 0.14: beyond the 1e-6 clip on both sides ...
    loc[:, 0, 0], loc[:, 1, 2], loc[:, 2, 3] = 5.0, 5.0, 5.0                         # ... at kept pixels
    loc[0] = -30.0                                                                   # frame 0: no kept pixel
    loc[1] = -30.0
    loc[1, H - 1, W - 2] = 4.0                                                       # frame 1: one kept pixel
    return buf, shape, loc


def _check_readout(props, counts, cls, reg, shape, keep, base, stride, img_shape, cfg, kw, what):
    """Device proposals against the statement's read-out of the same maps: same count, same order, boxes inside the f32 bound."""
    props, counts = props.cpu().numpy(), counts.cpu().numpy()
    stats = dict(empty=0, single=0, topk=0, post=0, maxn=0, aclip=0, iclip=0)
    for t in range(cls.shape[0]):
        r = R.proposals_statement(cls[t], reg[t], shape[t], keep[t], base, stride, kw['anchoring_means'], kw['anchoring_stds'], kw['target_means'],
                                  kw['target_stds'], img_shape, cfg['nms_pre'], cfg['nms_post'], cfg['max_num'], cfg['nms_thr'])
        ok_s, ok_i = R.readout_conditions(r, cfg['nms_thr'])
        assert ok_s and ok_i, 'the inputs do not force the selection in f32 (scores distinct %s, IoUs clear of the threshold %s)' % (ok_s, ok_i)
        n = len(r['props'])
        assert int(counts[t]) == n, (what, t, int(counts[t]), n)
        got = props[t, :n].astype(np.float64)
        assert (np.abs(got[:, 4] - r['props'][:, 4]) <= R.sigmoid_bound(r['props'][:, 4])).all(), (what, t, 'scores / order')
        _inside(got[:, :4], r['props'][:, :4], r['bound'], '%s frame %d boxes' % (what, t))
        assert (props[t, n:] == 0).all()
        full = R.proposals_statement(cls[t], reg[t], shape[t], keep[t], base, stride, kw['anchoring_means'], kw['anchoring_stds'], kw['target_means'],
                                     kw['target_stds'], img_shape, cfg['nms_pre'], 10 ** 6, 10 ** 6, cfg['nms_thr'])
        nk = int(keep[t].sum())
        stats['empty'] += nk == 0
        stats['single'] += nk == 1
        stats['topk'] += cfg['nms_pre'] > 0 and nk > cfg['nms_pre']
        stats['post'] += len(full['props']) > cfg['nms_post']
        stats['maxn'] += min(len(full['props']), cfg['nms_post']) > cfg['max_num']
        stats['aclip'] += bool((np.abs(shape[t][keep[t]] * np.array(kw['anchoring_stds'][2:])) > abs(np.log(1e-6))).any())
        stats['iclip'] += bool(n and ((got[:, :2] == 0).any() or (got[:, 2] == img_shape[1] - 1).any() or (got[:, 3] == img_shape[0] - 1).any()))
    return stats


@pytest.mark.parametrize('T', (2, 5))
@pytest.mark.parametrize('hw', MAPS)
def test_guided_proposals_on_prescribed_maps(hw, T):
    (H, W), thr, stride = hw, 0.3, 16
    img_shape = (H * stride - 7, W * stride - 5)
    base = R.base_square(stride, 2)
    buf, shape, loc = _prescribed(T, H, W, 900 + 10 * H + T, thr)
    keep_ref, amb = R.loc_mask_statement(loc[..., 0].numpy(), thr)
    assert not amb.any()
    bd, sd, ld = buf.to(DEV), shape.to(DEV), loc.to(DEV)
    keep = native.ga_loc_mask(ld, thr)
    assert np.array_equal(keep.cpu().numpy().astype(bool), keep_ref)
    cls_n, reg_n = buf[..., 0].numpy(), buf[..., 1:5].numpy()
    total = dict()
    for cfg in CFGS:
        args = (torch.from_numpy(base).float(), stride, KW['anchoring_means'], KW['anchoring_stds'], KW['target_means'], KW['target_stds'], img_shape,
                cfg['nms_pre'], cfg['nms_post'], cfg['max_num'], cfg['nms_thr'])
        p1, c1 = native.ga_rpn_proposals(bd[..., 0:1], bd[..., 1:5], sd, keep, *args)                       # cls, reg: slices of one buffer
        p2, c2 = native.ga_rpn_proposals(bd[..., 0:1].contiguous(), bd[..., 1:5].contiguous(), sd, keep, *args)
        assert torch.equal(p1, p2) and torch.equal(c1, c2), 'sliced and dense maps give different proposals'
        st = _check_readout(p1, c1, cls_n, reg_n, shape.numpy(), keep_ref, base, stride, img_shape, cfg, KW, 'T %d %dx%d %s' % (T, H, W, cfg))
        for k, v in st.items():
            total[k] = total.get(k, 0) + int(v)
        assert int(c1[0]) == 0 and int(c1[1]) == 1
    assert total['empty'] and total['single'], total
    if T > 2:
        assert all(total[k] for k in ('topk', 'post', 'maxn', 'aclip', 'iclip')), total


def test_guided_proposals_refusals():
    z = torch.zeros((1, 100, 100, 8), device=DEV)
    keep = torch.zeros((1, 100, 100), dtype=torch.uint8, device=DEV)
    with pytest.raises(native.HvrError, match='8192'):
        native.ga_rpn_proposals(z[..., 0:1], z[..., 1:5], z[..., 5:7], keep, [0, 0, 15, 15], 16, KW['anchoring_means'], KW['anchoring_stds'],
                                KW['target_means'], KW['target_stds'], (1600, 1600), 100, 10, 10, 0.7)
    z, keep = z[:, :5, :7].contiguous(), keep[:, :5, :7].contiguous()
    with pytest.raises(native.HvrError, match=r'\(-1\)'):
        native.ga_rpn_proposals(z[..., 0:1], z[..., 1:5], z[..., 5:7], keep, [0, 0, 15, 15], 16, KW['anchoring_means'], KW['anchoring_stds'],
                                KW['target_means'], KW['target_stds'], (80, 112), 100, 0, 10, 0.7)
    with pytest.raises(native.HvrError, match=r'\(-1\).*wh_ratio_clip'):
        native.ga_rpn_proposals(z[..., 0:1], z[..., 1:5], z[..., 5:7], keep, [0, 0, 15, 15], 16, KW['anchoring_means'], KW['anchoring_stds'],
                                KW['target_means'], KW['target_stds'], (80, 112), 100, 10, 10, 0.7, wh_ratio_clip=0.0)


# ------------------------------------------------------------------------------------------------ the head end to end
HEAD_KW = dict(in_channels=64, feat_channels=64, octave_base_scale=2, anchor_strides=[16], deformable_groups=4, loc_filter_thr=0.3, **KW)


def _head(mode, seed=77):
    head = hvrnet_amd.GARPNHead(**HEAD_KW)
    tg = torch.Generator().manual_seed(seed)
    thr = HEAD_KW['loc_filter_thr']
    with torch.no_grad():
        for m, std in ((head.rpn_conv, 1.4 / 24), (head.conv_loc, 2.0 / 8), (head.conv_shape, 4.0 / 8), (head.feature_adaption.conv_offset, 0.3),
                       (head.feature_adaption.conv_adaption, 1.4 / 24), (head.conv_cls, 2.0 / 8), (head.conv_reg, 3.0 / 8)):
            m.weight.copy_(torch.randn(m.weight.shape, generator=tg) * std)
            if m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=tg) * 0.1)
        head.conv_loc.bias.add_(float(np.log(thr / (1 - thr))) - 0.6)
    hvrnet_amd.set_compute_dtype(head, DTYPES[mode])
    return head.to(DEV).eval()


def _bracket(got, ref, bound, mode, what, out_f32=False):
    lo, hi = F.stored_bracket(ref, bound, mode, out_f32=out_f32)
    ratio, bad, worst = F.compare(got, lo, hi, ref)
    print('%s %s: worst |got - ref| / bracket = %.3f, %d of %d outside' % (what, mode, ratio, bad, ref.numel()))
    assert bad == 0, (what, mode, ratio, bad, worst)


@pytest.mark.parametrize('mode', F.MODES)
def test_head_forward_chain_and_proposals(mode):
    """C = 64, dg = 4, 2 frames of 80 x 112 (a 5 x 7 map).  GARPNHead.forward equals, bit for bit, the chain of public native calls; every
    link of that chain lies inside its statement's bound on the stored values of the link before (the statement chain); the proposals
    equal the statement's read-out of the device's own maps."""
    head = _head(mode)
    dt, dg, thr = DTYPES[mode], HEAD_KW['deformable_groups'], HEAD_KW['loc_filter_thr']
    tg = torch.Generator().manual_seed(5)
    x = F.store_true(torch.randn((2, 5, 7, 64), generator=tg).clamp(min=0), mode, 'act')
    xd = D.to_device_operand(x, mode, DEV)
    with torch.no_grad():
        cls, reg, shape, loc = (o[0] for o in head([xd.permute(0, 3, 1, 2)]))
        p = head.packed(xd.device)
        # the hand-made chain
        y = native.conv2d_nhwc(xd, p['conv'][0], p['conv'][1], relu=True, pad=1)
        ls = native.conv2d_nhwc(y, p['locshape'][0], p['locshape'][1], relu=False, out_f32=True)
        keep, om = native.ga_mask_offsets(loc=ls[..., 0:1], loc_filter_thr=thr, shape=ls[..., 1:3], w_off=p['off'])
        col = native.deform_im2col(y, om, 3, 3, 1, 1, 1, dg, False)
        z = native.deform_conv2d_nhwc(y, om, p['adapt'][0], p['adapt'][1], True, 1, 1, 1, dg, False)
        zf = native.cast(z, torch.float32) if mode == 'f16x2' else z
        o = native.masked_conv2d_nhwc(zf, p['heads'][0], p['heads'][1], keep)
    for a, b, what in ((cls, o[..., 0:1], 'cls'), (reg, o[..., 1:5], 'reg'), (shape, ls[..., 1:3], 'shape'), (loc, ls[..., 0:1], 'loc')):
        assert a.dtype == torch.float32 and tuple(a.shape) == (2, b.shape[3], 5, 7) and torch.equal(a.permute(0, 2, 3, 1), b), what
    # every link against its statement
    yv, wv = F.values(y).cpu(), F.values(p['conv'][0], 'weight').cpu()
    ref, mag, absxw = F.conv_statement(x, wv, p['conv'][1].cpu().double(), relu=True, pad=1, mode=mode)
    _bracket(yv, ref, F.mfma_bound(mag, absxw, 9 * 64, mode), mode, 'rpn_conv')
    ref, mag, absxw = F.conv_statement(yv, F.values(p['locshape'][0], 'weight').cpu(), p['locshape'][1].cpu().double(), mode=mode)
    _bracket(ls.cpu(), ref, F.mfma_bound(mag, absxw, 64, mode), mode, 'loc | shape', out_f32=True)
    lsn = ls.cpu().numpy()
    keep_ref, amb = R.loc_mask_statement(lsn[..., 0], thr)
    kn = keep.cpu().numpy().astype(bool)
    assert (kn == keep_ref)[~amb].all() and 0 < kn.sum() < kn.size, kn.mean()
    om_ref, om_bound = R.offsets_statement(lsn[..., 1:3], p['off'].cpu().numpy())
    _inside(om.cpu().numpy(), om_ref, om_bound, 'offsets')
    ref, bound = D.sampler_statement(yv, om.cpu(), 3, 3, 1, 1, 1, dg, False)
    lo, hi = D.stored_bracket(ref, bound, mode)
    assert F.compare(F.values(col).cpu(), lo, hi, ref)[1] == 0, 'sampler'
    ref, mag, absxw = F.gemm_statement(F.values(col).cpu(), F.values(p['adapt'][0], 'weight').cpu().reshape(64, -1), p['adapt'][1].cpu().double(), relu=True)
    _bracket(F.values(z).cpu().reshape(-1, 64), ref, F.mfma_bound(mag, absxw, 9 * 64, mode), mode, 'conv_adaption')
    zv = zf.double().cpu().numpy()
    assert mode != 'f16x2' or np.array_equal(zv, F.values(z).cpu().numpy())
    ref, bound = R.masked_conv_statement(zv, p['heads'][0].double().cpu().numpy(), p['heads'][1].double().cpu().numpy(), kn, 0)
    on = o.cpu().numpy()
    assert (on[~kn].view(np.uint32) == 0).all()
    _inside(on[kn], ref[kn], bound[kn], 'masked heads')
    assert float(np.abs(lsn[..., 1:3]).max()) > 0.5 and float(np.abs(om_ref).max()) > 0.1 and float(np.abs(on[kn]).max()) > 0.05
    # proposals: the statement's read-out of the DEVICE's own maps
    assert not amb.any(), 'a location logit of this seed lies inside the f32 sigmoid bound of the threshold'
    metas = [dict(img_shape=(80, 112, 3))] * 2
    base = R.base_square(16, HEAD_KW['octave_base_scale'])
    for cfg in CFGS[:2]:
        props, counts = head.get_bboxes_batched([cls], [reg], [shape], [loc], metas, cfg)
        _check_readout(props, counts, on[..., 0], on[..., 1:5], lsn[..., 1:3], kn, base, 16, (80, 112), cfg, KW, 'head %s %s' % (mode, cfg))
        lists = head.get_bboxes([cls], [reg], [shape], [loc], metas, cfg)
        assert [len(b) for b in lists] == counts.tolist() and all(torch.equal(b, props[i, :len(b)]) for i, b in enumerate(lists))


# ------------------------------------------------------------------------------------------------ a window with a GA-RPN head
HW, PAD = (120, 150), (128, 160)
T, NPROP = 3, 16
GA_HEAD = dict(type='GARPNHead', in_channels=1024, feat_channels=1024, octave_base_scale=8, scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0],
               anchor_strides=[16], anchoring_stds=[0.07, 0.07, 0.14, 0.14], target_stds=[0.07, 0.07, 0.11, 0.11], loc_filter_thr=0.01)


def _window_model(dtype):
    cfg = selsa_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(cfg.model.backbone, depth=50)
    cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
    cfg.model.rpn_head = GA_HEAD
    sd = {k: v for k, v in S.synth_state_dict('selsa', depth=50).items() if not k.startswith('rpn_head.')}
    sd.update(S.synth_ga_rpn_state_dict(1024, 4, GA_HEAD['loc_filter_thr']))
    return hvrnet_amd.build_model(cfg, sd, dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_ga_rpn_window_eager_and_graph_replay_are_equal():
    """A SelsaRCNN window whose rpn_head is a GARPNHead: eager, then captured and replayed (hvrnet_amd/graphs.py).  A host
    synchronisation inside the captured region would make the capture itself fail, so a graph that builds and replays IS the statement
    that the head enqueues and never waits; the replay equals the eager window bit for bit."""
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert type(model).__name__ == 'SelsaRCNN' and type(model.rpn_head) is hvrnet_amd.GARPNHead
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [torch.cat([S.synth_frame(10 * c + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV) for c in range(2)]
    with torch.no_grad():
        c4 = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
        outs = model.rpn_head([c4])
        props, counts = model.rpn_head.get_bboxes_batched(*outs, metas, model.test_cfg.rpn)
    loc = outs[3][0]
    keep = native.ga_loc_mask(loc.permute(0, 2, 3, 1), GA_HEAD['loc_filter_thr'])
    kept = float(keep.float().mean())
    print('kept fraction %.3f, proposals per frame %s' % (kept, counts.tolist()))
    assert 0.02 < kept < 0.98 and int(counts.min()) > 0 and float(outs[2][0].abs().max()) * 0.14 < 13.8
    assert bool(((outs[0][0][:, 0] == 0) == (keep == 0)).all()), 'the masked heads and the mask disagree about a pixel'
    first = [_eager(model, clip, metas) for clip in clips]
    again = [_eager(model, clip, metas) for clip in clips]
    g = GraphedClip(model, clips[0], metas, rescale=True)
    n_det = 0
    for rep in range(2):
        for clip, want, want2 in zip(clips, first, again):
            got = g.run(clip).result()
            assert len(got) == len(want)
            assert all(_same(a, b) for a, b in zip(want, want2)), 'two eager calls differ'
            assert all(_same(a, b) for a, b in zip(got, want)), 'graph replay differs from the eager window'
            for dets in got:                      # SelsaRCNN: one [k,5] array per class
                a = np.asarray(dets)
                assert a.ndim == 2 and a.shape[1] == 5 and np.isfinite(a).all()
                n_det += len(a)
    assert n_det > 0
