"""CPU tests of the Guided Anchoring RPN statements (tests/ga_rpn_refs.py): against the reference's own results
(tests/golden/g26_ga_rpn.npz, ga_rpn_modules.json), the fixture's own conditions asserted on the statement alone, every planted
mistake caught, and the host side of GARPNHead: keys, strict loading, the registry, the refusals, RPNHead untouched."""
import json
import os

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import registry, synthetic as S
from hvrnet_amd.config import hvr_config
from tests import ga_rpn_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, 'golden', 'g26_ga_rpn.npz'))
MODULES = json.load(open(os.path.join(HERE, 'golden', 'ga_rpn_modules.json')))
KW = MODULES['cases'][0]['kwargs']
CASES = ('a', 'b', 'c')
STRIDE = 16
BASE = R.base_square(STRIDE, KW['octave_base_scale'])


def _frames(name):
    img_h, img_w, thr, nms_pre, nms_post, max_num, nms_thr = Z[name + '.meta'].tolist()
    cfg = dict(img_shape=(img_h, img_w), nms_pre=int(nms_pre), nms_post=int(nms_post), max_num=int(max_num), nms_thr=nms_thr)
    T = Z[name + '.cls'].shape[0]
    return thr, cfg, T


def _readout(name, t, keep, cfg, mistake=None):
    return R.proposals_statement(Z[name + '.cls'][t, ..., 0], Z[name + '.reg'][t], Z[name + '.shape'][t], keep, BASE, STRIDE, KW['anchoring_means'],
                                 KW['anchoring_stds'], KW['target_means'], KW['target_stds'], cfg['img_shape'], cfg['nms_pre'], cfg['nms_post'],
                                 cfg['max_num'], cfg['nms_thr'], mistake=mistake)


def test_base_square_is_the_reference_grid():
    assert BASE.tolist() == [-8.0, -8.0, 23.0, 23.0] and R.base_square(16, 8).tolist() == [-56.0, -56.0, 71.0, 71.0]
    for name in CASES:
        H, W = Z[name + '.cls'].shape[1:3]
        assert np.array_equal(R.grid_squares(BASE, H, W, STRIDE), Z[name + '.squares'].astype(np.float64))


@pytest.mark.parametrize('name', CASES)
def test_mask_and_anchors_against_the_reference(name):
    thr, cfg, T = _frames(name)
    n_clip = 0
    for t in range(T):
        keep, amb = R.loc_mask_statement(Z[name + '.loc'][t, ..., 0], thr)
        assert not amb.any(), 'fixture condition: a loc logit within the f32 sigmoid bound of the threshold'
        assert np.array_equal(keep.reshape(-1), Z['%s.f%d.mask' % (name, t)].astype(bool)), 'mask'
        an, ean, idx = R.guided_anchors_statement(Z[name + '.shape'][t], keep, BASE, STRIDE, KW['anchoring_means'], KW['anchoring_stds'])
        ref = Z['%s.f%d.anchors' % (name, t)].astype(np.float64)
        assert an.shape == ref.shape and (np.abs(an - ref) <= ean).all(), float((np.abs(an - ref) / np.maximum(ean, 1e-30)).max())
        n_clip += int((np.abs(Z[name + '.shape'][t].reshape(-1, 2)[idx] * np.array(KW['anchoring_stds'][2:])) > abs(np.log(1e-6))).sum())
    assert n_clip > 0, 'fixture condition: the 1e-6 clip acts on a kept pixel'


def test_mask_condition_holds_in_the_coarsest_mode():
    """Fixture condition: every loc logit is further from logit(thr) than a bf16 rounding of the logit (2^-9 relative) plus the f32
    sigmoid bound could move it -- a mask made from these maps is forced, whatever the mode that stored them (exact zeros at thr 0.5
    are stored exactly in every mode)."""
    for name in CASES:
        thr = _frames(name)[0]
        loc = Z[name + '.loc'][..., 0].astype(np.float64)
        t = float(np.float32(thr))
        for d in (-1.0, 1.0):
            s = R.sigmoid(loc * (1.0 + d * 2.0 ** -9))
            near = (np.abs(s - t) <= R.sigmoid_bound(s)) & ~((loc == 0.0) & (t == 0.5))
            assert not near.any()
            assert np.array_equal(s >= t, R.sigmoid(loc) >= t)
    assert (Z['c.loc'] == 0.0).sum() >= 4, 'the equality case of >= is in the fixture'


@pytest.mark.parametrize('name', CASES)
def test_readout_against_the_reference(name):
    thr, cfg, T = _frames(name)
    seen = dict(topk=0, post=0, maxn=0, clip=0, single=0)
    for t in range(T):
        keep = Z['%s.f%d.mask' % (name, t)].astype(bool).reshape(Z[name + '.cls'].shape[1:3])
        r = _readout(name, t, keep, cfg)
        ok_s, ok_i = R.readout_conditions(r, cfg['nms_thr'])
        assert ok_s, 'fixture condition: candidate scores distinct by more than their bounds'
        assert ok_i, 'fixture condition: no candidate pair with an IoU within 1e-5 of nms_thr'
        ref = Z['%s.f%d.proposals' % (name, t)].astype(np.float64)
        assert r['props'].shape == ref.shape, (r['props'].shape, ref.shape)
        assert (np.abs(r['props'][:, 4] - ref[:, 4]) <= R.sigmoid_bound(ref[:, 4])).all(), 'scores (hence the order)'
        assert (np.abs(r['props'][:, :4] - ref[:, :4]) <= r['bound']).all(), float((np.abs(r['props'][:, :4] - ref[:, :4]) - r['bound']).max())
        assert (np.diff(r['props'][:, 4]) < 0).all()
        seen['topk'] += int(cfg['nms_pre'] > 0 and keep.sum() > cfg['nms_pre'])
        seen['single'] += int(keep.sum() == 1)
        seen['clip'] += int(((r['props'][:, :4] == 0).any() or (r['props'][:, 2] == cfg['img_shape'][1] - 1).any()))
        full = _readout(name, t, keep, dict(cfg, nms_post=10 ** 6, max_num=10 ** 6))
        seen['post'] += int(len(full['props']) > cfg['nms_post'])
        seen['maxn'] += int(min(len(full['props']), cfg['nms_post']) > cfg['max_num'])
    if name == 'a':
        assert seen['topk'] and seen['maxn'] and seen['post'] and seen['clip'], seen
    if name == 'b':
        assert seen['single'], seen
    if name == 'c':
        assert seen['post'], seen


def test_no_kept_pixel_gives_no_proposal():
    r = _readout('a', 0, np.zeros((5, 7), bool), _frames('a')[1])
    assert r['props'].shape == (0, 5) and len(r['pixels']) == 0


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_planted_mistake_is_caught(mistake):
    caught = 0
    if mistake in R.MASK_MISTAKES:
        for name in CASES:
            thr, cfg, T = _frames(name)
            for t in range(T):
                keep = R.loc_mask_statement(Z[name + '.loc'][t, ..., 0], thr, mistake)[0]
                caught += int(not np.array_equal(keep.reshape(-1), Z['%s.f%d.mask' % (name, t)].astype(bool)))
    elif mistake in R.CONV_MISTAKES:
        g = np.random.default_rng(5)
        x, w, b = g.standard_normal((3, 5, 7, 64)), g.standard_normal((5, 1, 1, 64)) / 8, g.standard_normal(5)
        keep = g.random((3, 5, 7)) < 0.5
        assert not np.array_equal(keep[0], keep[1])
        ref, bound = R.masked_conv_statement(x, w, b, keep, 0)
        assert (ref[~keep] == 0).all() and (bound[~keep] == 0).all() and (ref[keep] != 0).all()
        bad = R.masked_conv_statement(x, w, b, keep, 0, mistake)[0]
        caught += int((np.abs(bad - ref) > bound).any())
    else:
        for name in CASES:
            thr, cfg, T = _frames(name)
            for t in range(T):
                keep = Z['%s.f%d.mask' % (name, t)].astype(bool).reshape(Z[name + '.cls'].shape[1:3])
                ref = Z['%s.f%d.proposals' % (name, t)].astype(np.float64)
                r = _readout(name, t, keep, cfg, mistake)
                if mistake in R.ANCHOR_MISTAKES:
                    an, ean, _ = R.guided_anchors_statement(Z[name + '.shape'][t], keep, BASE, STRIDE, KW['anchoring_means'], KW['anchoring_stds'], mistake)
                    caught += int((np.abs(an - Z['%s.f%d.anchors' % (name, t)]) > ean).any())
                caught += int(r['props'].shape != ref.shape or bool((np.abs(r['props'][:, :4] - ref[:, :4]) > r['bound']).any())
                              or bool((np.abs(r['props'][:, 4] - ref[:, 4]) > R.sigmoid_bound(ref[:, 4])).any()))
    assert caught > 0, '%s passes every check' % mistake


def test_offsets_statement():
    g = np.random.default_rng(3)
    shape, w = g.standard_normal((2, 3, 4, 2)).astype(np.float32), g.standard_normal((72, 2)).astype(np.float32)
    om, bound = R.offsets_statement(shape, w)
    f32 = (w[:, 0] * shape[..., 0:1] + w[:, 1] * shape[..., 1:2]).astype(np.float64)       # numpy's own f32 evaluation: two products, one add
    assert om.shape == (2, 3, 4, 72) and (np.abs(f32 - om) <= bound).all() and (bound > 0).all()


def test_masked_conv_statement_is_the_dense_conv_under_the_mask():
    g = np.random.default_rng(4)
    x, w, b = g.standard_normal((2, 5, 7, 8)), g.standard_normal((3, 3, 3, 8)), g.standard_normal(3)
    keep = g.random((2, 5, 7)) < 0.6
    ref, _ = R.masked_conv_statement(x, w, b, keep, 1)
    dense = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2), torch.from_numpy(b), padding=1)
    dense = dense.permute(0, 2, 3, 1).numpy()
    assert np.allclose(ref[keep], dense[keep], rtol=1e-12, atol=1e-12) and (ref[~keep] == 0).all()


def test_forward_chain_statement_with_zero_offsets_is_the_plain_chain():
    """With conv_offset = 0 the deformable conv is the plain 3x3 conv: the f64 chain must equal torch's own convs; and the masked heads
    are zero exactly where the location score is below the threshold.  (The sampler rounds its position add in f32: offsets of zero
    keep it exact.)"""
    g = np.random.default_rng(8)
    B, H, W, C, dg, thr = 2, 5, 7, 16, 2, 0.4
    x = np.maximum(g.standard_normal((B, H, W, C)), 0)
    prm = dict(rpn_conv=(g.standard_normal((C, 3, 3, C)) / 12, g.standard_normal(C) * 0.1), loc=(g.standard_normal((1, 1, 1, C)) / 2, np.array([-0.4])),
               shape=(g.standard_normal((2, 1, 1, C)) / 4, g.standard_normal(2) * 0.1), off=np.zeros((dg * 18, 2)),
               adapt=g.standard_normal((C, 3, 3, C)) / 12, cls=(g.standard_normal((1, 1, 1, C)) / 4, np.array([0.3])),
               reg=(g.standard_normal((4, 1, 1, C)) / 4, g.standard_normal(4) * 0.1))
    r = R.forward_chain_statement(x, prm, thr, dg)

    def conv(a, w, b, pad):
        y = torch.nn.functional.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2),
                                       None if b is None else torch.from_numpy(b), padding=pad)
        return y.permute(0, 2, 3, 1).numpy()
    y = np.maximum(conv(x, *prm['rpn_conv'], 1), 0)
    loc = conv(y, *prm['loc'], 0)[..., 0]
    keep = 1 / (1 + np.exp(-loc)) >= float(np.float32(thr))
    z = np.maximum(conv(y, prm['adapt'], None, 1), 0)
    assert np.allclose(r['y'], y, atol=1e-12) and np.allclose(r['loc'], loc, atol=1e-12) and np.array_equal(r['keep'], keep) and 0 < keep.mean() < 1
    assert (r['om'] == 0).all() and np.allclose(r['z'], z, atol=1e-12) and np.allclose(r['shape'], conv(y, *prm['shape'], 0), atol=1e-12)
    assert np.allclose(r['cls'][keep], conv(z, *prm['cls'], 0)[..., 0][keep], atol=1e-12) and (r['cls'][~keep] == 0).all()
    assert np.allclose(r['reg'][keep], conv(z, *prm['reg'], 0)[keep], atol=1e-12) and (r['reg'][~keep] == 0).all()
    prm['off'] = g.standard_normal((dg * 18, 2)) * 0.5
    moved = R.forward_chain_statement(x, prm, thr, dg)
    assert np.abs(moved['z'] - r['z']).max() > 1e-3 and np.array_equal(moved['keep'], r['keep'])


# ------------------------------------------------------------------------------------------------ the head's host side
def test_state_dict_keys_and_strict_load():
    for case in MODULES['cases']:
        head = registry.build_from_cfg(dict(case['kwargs'], type='GARPNHead'), registry.HEADS)
        assert type(head) is hvrnet_amd.GARPNHead
        assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == case['keys']
        C = case['kwargs']['in_channels']
        if C == 64:
            sd = S.synth_ga_rpn_state_dict(C, case['kwargs']['deformable_groups'], prefix='')
            head.load_state_dict(sd, strict=True)
            assert all(torch.equal(v, sd[k]) for k, v in head.state_dict().items())
    assert 'feature_adaption.conv_adaption.bias' not in dict(MODULES['cases'][0]['keys']) and 'feature_adaption.conv_offset.bias' not in dict(MODULES['cases'][0]['keys'])


def test_init_weights_follow_the_reference():
    head = hvrnet_amd.GARPNHead(64, feat_channels=64, anchor_strides=[16])
    head.init_weights()
    assert float(head.conv_loc.bias) == pytest.approx(-np.log(99.0)) and float(head.conv_cls.bias.abs().max()) == 0
    assert 0.05 < float(head.feature_adaption.conv_offset.weight.std()) < 0.2 and float(head.rpn_conv.weight.std()) < 0.02


def test_refusals():
    ok = dict(type='GARPNHead', in_channels=64, feat_channels=64, anchor_strides=[16])
    registry.build_from_cfg(ok, registry.HEADS)
    for bad, word in ((dict(feat_channels=128), 'in_channels'), (dict(anchor_strides=[8, 16]), 'single-level'),
                      (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False)), 'softmax'),
                      (dict(in_channels=72, feat_channels=72), 'sampler'), (dict(deformable_groups=16), 'sampler')):
        with pytest.raises(NotImplementedError, match=word):
            registry.build_from_cfg(dict(ok, **bad), registry.HEADS)
    head = registry.build_from_cfg(ok, registry.HEADS)
    maps = [[torch.zeros(1, c, 5, 7)] for c in (1, 4, 2, 1)]
    metas = [dict(img_shape=(80, 112, 3))]
    base = dict(nms_pre=10, nms_post=10, max_num=10, nms_thr=0.7)
    for cfg, word in ((dict(base, nms_across_levels=True), 'nms_across_levels'), (dict(base, min_bbox_size=2), 'min_bbox_size')):
        with pytest.raises(NotImplementedError, match=word):
            head.get_bboxes_batched(*maps, metas, cfg)
    with pytest.raises(NotImplementedError, match='single-level'):
        head.get_bboxes_batched(*[m * 2 for m in maps], metas, base)
    with pytest.raises(NotImplementedError, match='GPU only'):
        head([torch.zeros(1, 64, 5, 7)])
    for fn in (head.loss, head.loss_train, head.forward_train_fused, head.forward_train_nhwc):
        with pytest.raises(NotImplementedError, match='GARPNHead'):
            fn()
    with pytest.raises(NotImplementedError):
        hvrnet_amd.MaskedConv2d(8, 2, 1)(torch.zeros(1, 8, 3, 3), torch.ones(1, 3, 3))


def test_detector_with_a_ga_rpn_head_builds_and_loads_strictly():
    cfg = hvr_config()
    kw = dict(MODULES['cases'][1]['kwargs'], type='GARPNHead')
    cfg.model.backbone = dict(cfg.model.backbone, depth=50)
    cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
    cfg.model.rpn_head = kw
    model = hvrnet_amd.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    assert type(model.rpn_head) is hvrnet_amd.GARPNHead
    sd = {k: v for k, v in S.synth_state_dict('hvr', depth=50).items() if not k.startswith('rpn_head.')}
    sd.update(S.synth_ga_rpn_state_dict(1024, 4))
    model.load_state_dict(sd, strict=True)
    with pytest.raises(NotImplementedError, match='GARPNHead is inference only'):
        hvrnet_amd.detectors._need_trainable_rpn(model.rpn_head)


def test_rpn_head_of_the_stock_config_is_untouched():
    cfg = hvr_config()
    head = registry.build_from_cfg(cfg.model.rpn_head, registry.HEADS)
    assert type(head) is hvrnet_amd.RPNHead and not getattr(head, 'inference_only', False)
    assert list(head.state_dict().keys()) == ['rpn_conv.weight', 'rpn_conv.bias', 'rpn_cls.weight', 'rpn_cls.bias', 'rpn_reg.weight', 'rpn_reg.bias']
    sd = S.synth_state_dict('hvr', depth=50)
    assert sorted(k for k in sd if k.startswith('rpn_head.')) == sorted('rpn_head.' + k for k in head.state_dict())
    hvrnet_amd.detectors._need_trainable_rpn(head)
