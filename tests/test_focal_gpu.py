"""The sigmoid focal loss kernels (hvrnet_amd/csrc/focal.hip) against the f64 statements of tests/focal_refs.py, through native.*, the
autograd op, the FocalLoss module, the sampling-free anchor targets and one SelsaRCNN training iteration with a focal RPN.

Every bound is the derived one of focal_refs (nothing is measured against the device), every element of every output is compared and
nothing is excluded.  Each comparison prints `RATIO <kernel> <dtype> <worst error / bound>` (pytest -s shows it)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, ops, synthetic as S  # noqa: E402
from hvrnet_amd import targets as T  # noqa: E402
from hvrnet_amd import train_ops as TO  # noqa: E402
from tests import focal_refs as R  # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'half'}
GA = [(2.0, 0.25), (0.0, 0.5), (1.5, 0.75)]
SHAPES = [(1, 1, 1), (7, 1, 1), (5, 3, 3), (5, 3, 7), (64, 80, 80), (257, 12, 13), (1000, 31, 32)]


def check(kernel, dtype, got, ref, bound):
    """Every element of `got` within `bound` of `ref`; prints the worst error / bound."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %s %.4g' % (kernel, NAMES.get(dtype, dtype), worst))
    assert bool(torch.isfinite(got.double()).all()), kernel
    assert worst <= 1.0, '%s: %d of %d elements over the bound, worst error / bound %g' % (kernel, int((ratio > 1).sum()), ratio.numel(), worst)


def smallest_partly_filled(C=3):
    """The smallest N at C columns for which the library cuts at least 3 workgroups and the last one holds fewer rows than the others."""
    for N in range(1, 100000):
        S_ = native.focal_loss_splits(N, C)
        Sr, rows = R.focal_loss_splits(N, C)
        assert S_ == Sr
        if S_ >= 3 and N % rows:
            return N
    raise AssertionError('no such shape')


# ------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: NAMES[d])
@pytest.mark.parametrize('N,C,ldl', SHAPES, ids=lambda v: str(v))
def test_elementwise_forward_and_backward_against_f64(N, C, ldl, dtype):
    """(N, C, ldl) with and without pitch, ldl % 4 != 0 (the scalar form), C % 4 == 0 at a 16-byte pitch (4 f32 / 8 half per lane), more
    rows than one workgroup step; targets 0, 1, C and -1; the normal, saturated and extreme families (both sides of x = -87.3)."""
    t = R.targets_for(N, C, seed=N + C).to(DEV)
    for fi, family in enumerate(R.FAMILIES):
        gamma, alpha = GA[fi]
        for ga in ([(gamma, alpha)] if family != 'normal' else GA):
            xf = R.logits_family(family, N, ldl, seed=N * 7 + ldl, dtype=dtype).to(DEV)
            x = xf[:, :C]
            loss = native.sigmoid_focal_loss_fwd(x, t, *ga)
            ref, bound = R.focal_statement(x, t, *ga)
            assert loss.shape == (N, C) and loss.dtype == torch.float32 and bool(torch.isfinite(loss).all())
            check('focal_fwd.%s' % family, dtype, loss, ref['l'], bound['l'])
            d_loss = (0.5 + torch.rand((N, C), generator=torch.Generator().manual_seed(N))).to(DEV)
            dx = native.sigmoid_focal_loss_bwd(x, t, d_loss, *ga)
            dref, dbound = R.focal_bwd_statement(x, t, d_loss, *ga)
            check('focal_bwd.%s' % family, dtype, dx, dref, dbound)
            dead = t < 0
            assert bool((loss[dead] == 0).all() and (dx[dead] == 0).all())
            if family == 'extreme' and N * C >= 9:
                assert float(ref['l'].max()) > 20.0          # x = -100 on a positive: the loss follows -alpha x past the reference's clamp


# ------------------------------------------------------------------------------------------------ reduced form
def _fused_shapes():
    return SHAPES + [(4099, 3, 3)]


@pytest.mark.parametrize('N,C,ldl', _fused_shapes() + [('partly', 3, 3)], ids=lambda v: str(v))
def test_reduced_form_against_f64(N, C, ldl):
    """The elementwise shapes, (4099, 3, 3) and the smallest shape the library cuts into at least 3 workgroups with a partly filled last
    one; w given / null; avg from the host / from the device (a count of 0 clamps to 1); rows with w = 0 or t < 0 give exactly zero;
    pitch columns are zero; two calls are bit-equal."""
    if N == 'partly':
        N = smallest_partly_filled(C)
        S_, rows = R.focal_loss_splits(N, C)
        assert native.focal_loss_splits(N, C) == S_ >= 3 and 0 < N - (S_ - 1) * rows < rows
    t = R.targets_for(N, C, seed=N + C).to(DEV)
    w = R.row_weights(N, seed=N).to(DEV)
    for family, (gamma, alpha), use_w, dev_avg in (('normal', GA[0], True, None), ('normal', GA[2], False, 5), ('extreme', GA[0], True, 0),
                                                   ('saturated', GA[1], False, None)):
        xf = R.logits_family(family, N, ldl, seed=N * 7 + ldl).to(DEV)
        x = xf[:, :C]
        counts = None if dev_avg is None else torch.tensor([dev_avg, 77], dtype=torch.int32, device=DEV)
        avg = 7.5 if dev_avg is None else float(max(dev_avg, 1))                    # a device count of 0 clamps to 1
        call = lambda: native.focal_loss(x, t, w if use_w else None, gamma, alpha, 1.5, 7.5 if counts is None else 123.0, counts)   # noqa: E731
        out1, d = call()
        ref, bound = R.focal_loss_statement(xf, C, t, w if use_w else None, gamma, alpha, 1.5, avg)
        assert d.shape == (N, ldl)
        check('focal_loss.out1.%s' % family, torch.float32, out1[0], ref['out1'], bound['out1'])
        check('focal_loss.d.%s' % family, torch.float32, d, ref['d'], bound['d'])
        assert bool((d[:, C:] == 0).all())                                          # pitch columns
        dead = (t < 0) | ((w == 0) if use_w else torch.zeros_like(t, dtype=torch.bool))
        assert bool((d[dead] == 0).all())
        out1b, db = call()
        assert torch.equal(out1, out1b) and torch.equal(d, db)
    # rows that carry nothing give exactly 0 loss
    x = R.logits_family('normal', N, ldl, seed=3).to(DEV)[:, :C]
    out1, d = native.focal_loss(x, t, torch.zeros(N, device=DEV), 2.0, 0.25, 1.0, 1.0)
    assert float(out1[0]) == 0.0 and not bool(d.any())
    out1, d = native.focal_loss(x, torch.full((N,), -1, dtype=torch.long, device=DEV), None, 2.0, 0.25, 1.0, 1.0)
    assert float(out1[0]) == 0.0 and not bool(d.any())


def test_reduced_form_replays_from_a_graph():
    N, C, ldl = 257, 12, 13
    x = R.logits_family('normal', N, ldl, seed=1).to(DEV)[:, :C]
    t, w = R.targets_for(N, C, seed=2).to(DEV), R.row_weights(N, seed=3).to(DEV)
    counts = torch.tensor([9, 0], dtype=torch.int32, device=DEV)
    run = lambda: native.focal_loss(x, t, w, 2.0, 0.25, 1.0, 1.0, counts)     # noqa: E731
    want = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out1, d = run()
    for _ in range(2):
        out1.fill_(3)
        d.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out1, want[0]) and torch.equal(d, want[1])


# ------------------------------------------------------------------------------------------------ RPN form
@pytest.mark.parametrize('weights', [(1.0, 1.0), (2.0, 0.5)], ids=lambda v: 'w%g_%g' % v)
@pytest.mark.parametrize('counts', [(0, 9), (7, 40)], ids=lambda c: 'c%d_%d' % c)
@pytest.mark.parametrize('H,W,A,ld', [(6, 5, 12, 64), (4, 5, 3, 15), (1, 1, 1, 5)], ids=lambda v: str(v))
def test_rpn_form_against_f64(H, W, A, ld, counts, weights):
    for family, (gamma, alpha) in zip(R.FAMILIES, GA):
        c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in R.rpn_focal_case(H, W, A, ld, counts, seed=H * W + A, family=family).items()}
        out2, d_o = native.rpn_focal_loss(c['o'], A, c['labels'], c['label_w'], c['bbox_t'], c['bbox_w'], c['counts'], c['beta'], gamma, alpha, *weights)
        ref, bound = R.rpn_focal_statement(gamma=gamma, alpha=alpha, w_cls=weights[0], w_bbox=weights[1], **dict(c, counts=c['counts'].tolist()))
        check('rpn_focal.loss.%s' % family, torch.float32, out2, ref['out2'], bound['out2'])
        check('rpn_focal.d_o.%s' % family, torch.float32, d_o, ref['d_o'], bound['d_o'])
        assert bool((d_o[:, 5 * A:] == 0).all())
        out2b, d_ob = native.rpn_focal_loss(c['o'], A, c['labels'], c['label_w'], c['bbox_t'], c['bbox_w'], c['counts'], c['beta'], gamma, alpha, *weights)
        assert torch.equal(out2, out2b) and torch.equal(d_o, d_ob)


# ------------------------------------------------------------------------------------------------ autograd and module
def test_autograd_op_and_module():
    N, C = 64, 80
    x0 = R.logits_family('normal', N, C, seed=8).to(DEV)
    t, w = R.targets_for(N, C, seed=9).to(DEV), R.row_weights(N, seed=10).to(DEV)
    ref, bound = R.focal_statement(x0, t, 2.0, 0.25)
    x = x0.clone().requires_grad_(True)
    loss = ops.sigmoid_focal_loss(x, t, 2.0, 0.25)
    loss.sum().backward()
    check('op.loss', torch.float32, loss.detach(), ref['l'], bound['l'])
    check('op.grad', torch.float32, x.grad, ref['g'], bound['g'] + R.U * ref['g'].abs())
    s = ops.SigmoidFocalLoss(2.0, 0.25)(x0, t)
    assert abs(float(s) - float(ref['l'].sum())) <= 1e-5 * float(ref['l'].sum())
    for red, avg_factor, avg, lw in (('mean', 11.0, 11.0, 2.0), ('mean', None, float(N * C), 1.0), ('sum', None, 1.0, 0.5)):
        m = hvrnet_amd.FocalLoss(gamma=1.5, alpha=0.75, reduction=red, loss_weight=lw)
        x = x0.clone().requires_grad_(True)
        out = m(x, t, w, avg_factor=avg_factor)
        (out * 3.0).backward()
        r, b = R.focal_loss_statement(x0, C, t, w, 1.5, 0.75, lw, avg)
        check('module.%s' % red, torch.float32, out.detach(), r['out1'], b['out1'])
        check('module.%s.grad' % red, torch.float32, x.grad, 3.0 * r['d'], 3.0 * b['d'] + R.U * 3.0 * r['d'].abs())
    m = hvrnet_amd.FocalLoss(gamma=1.5, alpha=0.75, reduction='mean', loss_weight=2.0)
    none = m(x0, t, w, reduction_override='none')
    r, b = R.focal_statement(x0, t, 1.5, 0.75)
    check('module.none', torch.float32, none, 2.0 * w.double()[:, None] * r['l'], 2.0 * w.double()[:, None] * b['l'] + 2 * R.U * (2.0 * w.double()[:, None] * r['l']).abs())
    over = m(x0, t, w, reduction_override='sum')
    r, b = R.focal_loss_statement(x0, C, t, w, 1.5, 0.75, 2.0, 1.0)
    check('module.override_sum', torch.float32, over, r['out1'], b['out1'])


# ------------------------------------------------------------------------------------------------ targets
def test_sampling_free_anchor_targets_equal_the_golden_and_the_host_restatement():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'focal.npz'))
    anchors, gts = torch.as_tensor(g['at.anchors']).to(DEV), torch.as_tensor(g['at.gt_bboxes']).to(DEV)
    meta = dict(img_shape=tuple(int(v) for v in g['at.img_shape']), pad_shape=(64, 80, 3), scale_factor=1.0, flip=False)
    lab, lw, bt, bw, counts = T.anchor_target_single(anchors, None, gts, meta, [0., 0., 0., 0.], [1., 1., 1., 1.], R.AT_CFG, sampling=False)
    hl, hw_, hbt, hbw, (npos, nneg) = R.anchor_target_host(anchors, None, gts, meta['img_shape'], R.AT_CFG)
    assert counts.tolist() == [npos, nneg] == [int(g['at.num_pos']), int(g['at.num_neg'])]
    for got, host, gold in ((lab, hl, g['at.labels']), (lw, hw_, g['at.label_weights']), (bw, hbw, g['at.bbox_weights'])):
        assert np.array_equal(got.cpu().numpy(), gold) and torch.equal(got.cpu(), host)
    assert np.allclose(bt.cpu().numpy(), g['at.bbox_targets'], rtol=0, atol=1e-6) and torch.allclose(bt.cpu(), hbt, rtol=0, atol=1e-6)
    a = g['at.anchors']
    ins = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < meta['img_shape'][1]) & (a[:, 3] < meta['img_shape'][0])
    lwn = lw.cpu().numpy()
    assert (~ins).any() and (lwn[~ins] == 0).all() and int(ins.sum()) > npos + nneg and int((lwn > 0).sum()) == npos + nneg
    # the list form and the sampler object: the same set, positives first, each ascending
    out = T.anchor_target([[anchors]], None, [gts], [meta], [0., 0., 0., 0.], [1., 1., 1., 1.], R.AT_CFG, sampling=False)
    assert torch.equal(out[0][0][0], lab) and (out[4], out[5]) == (npos, nneg)
    ar = T.build_assigner(R.AT_CFG['assigner']).assign(anchors, gts, None, None, valid=torch.as_tensor(ins).to(DEV).to(torch.uint8))
    res = T.build_sampler(dict(type='PseudoSampler')).sample(ar, anchors, gts)
    assert res.pos_inds.tolist() == torch.nonzero(ar.gt_inds > 0).flatten().tolist() and res.neg_inds.tolist() == torch.nonzero(ar.gt_inds == 0).flatten().tolist()
    with pytest.raises(NotImplementedError):
        T.anchor_target([[anchors]], None, [gts], [meta], [0.] * 4, [1.] * 4, R.AT_CFG, gt_labels_list=[torch.ones(2, dtype=torch.long)], sampling=False)


# ------------------------------------------------------------------------------------------------ refused arguments
def test_refused_arguments_name_the_constraint():
    lib = native.lib()
    x = torch.zeros((4, 8), device=DEV)
    t = torch.zeros(4, dtype=torch.long, device=DEV)
    out = torch.zeros((4, 8), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda v: ctypes.c_void_p(v.data_ptr())     # noqa: E731

    def fwd(ldl=8, C=8, gamma=2.0, alpha=0.25, dtype=0):
        return lib.hvr_sigmoid_focal_loss_fwd(p(x), ldl, p(t), 4, C, gamma, alpha, dtype, p(out), None)

    def fused(ldl=8, gamma=2.0, alpha=0.25, ws_bytes=256, avg=1.0):
        return lib.hvr_focal_loss(p(x), ldl, p(t), None, 4, 8, gamma, alpha, 1.0, avg, None, p(ws), ws_bytes, p(out), p(out), None)

    for call, word in ((lambda: fwd(ldl=7), 'ldl >= C'), (lambda: fwd(gamma=-0.5), 'gamma >= 0'), (lambda: fwd(alpha=1.5), 'alpha <= 1'),
                       (lambda: fwd(C=0), 'N, C >= 1'), (lambda: fwd(dtype=3), 'split-half'), (lambda: fused(ldl=7), 'ldl >= C'),
                       (lambda: fused(gamma=-1.0), 'gamma >= 0'), (lambda: fused(alpha=-0.1), '0 <= alpha'), (lambda: fused(ws_bytes=0), 'ws_bytes'),
                       (lambda: fused(avg=0.0), 'avg > 0')):
        assert call() != 0
        assert word in lib.hvr_last_error().decode(), (word, lib.hvr_last_error().decode())
    with pytest.raises(native.HvrError, match='ws_bytes'):
        native.focal_loss(x, t, ws=torch.zeros(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(native.HvrError, match='gamma >= 0'):
        native.rpn_focal_loss(torch.zeros((1, 5), device=DEV), 1, t[:1], x[:1, 0], x[:1, :4], x[:1, :4], torch.zeros(2, dtype=torch.int32, device=DEV),
                              1.0, -2.0, 0.25)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
def test_selsa_trains_with_a_focal_rpn(monkeypatch):
    """SelsaRCNN.forward_train with rpn_head.loss_cls = FocalLoss: the RPN terms equal the statement on the captured head output and the
    sampling-free targets (all assigned anchors, divided by the positive count), the RPN convs receive gradients, a second call gives the
    same bits.  Anchor scales 1 .. 4 x 16 px so that anchors lie inside a 64 x 64 frame (twelve per position, as the synthetic weights)."""
    from hvrnet_amd.config import selsa_train_config
    Tn, hw = 3, (64, 64)
    cfg = selsa_train_config(nms_post=8, rcnn_sampler_num=4, t_dim=Tn)
    cfg.model.backbone['depth'] = 50
    cfg.model.shared_head['depth'] = 50
    cfg.model.rpn_head.update(anchor_scales=[1, 1.5, 2, 4], loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
                              loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=0.5))
    model = hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, S.synth_state_dict('selsa', depth=50), torch.float32, DEV))
    assert model.rpn_head.sampling is False
    seen = []
    real = TO.rpn_focal_loss

    def spy(o, A, labels, label_w, bbox_t, bbox_w, counts, **kw):
        seen.append(dict(o=o.detach().clone(), A=A, labels=labels, label_w=label_w, bbox_t=bbox_t, bbox_w=bbox_w, counts=counts.tolist(), kw=kw))
        return real(o, A, labels, label_w, bbox_t, bbox_w, counts, **kw)

    monkeypatch.setattr(TO, 'rpn_focal_loss', spy)
    g = torch.Generator().manual_seed(91)
    imgs = (torch.randn((Tn, 3) + hw, generator=g) * 50.0).to(DEV)
    metas = [dict(img_shape=hw + (3,), pad_shape=hw + (3,), scale_factor=1.0, flip=False) for _ in range(Tn)]
    gt_b = torch.tensor([[8., 8., 39., 39.], [30., 20., 60., 50.]]).to(DEV)
    gt_l = torch.tensor([5, 12]).to(DEV)
    keys = dict(rcnn=[torch.rand(2 + 8, generator=g).to(DEV) for _ in range(Tn)])

    def step():
        return model(imgs, metas, return_loss=True, gt_bboxes=[gt_b] * Tn, gt_labels=[gt_l] * Tn, keys=keys)

    got = step()
    losses = [v if isinstance(v, torch.Tensor) else sum(v) for k, v in got.items() if 'loss' in k]
    assert len(losses) >= 4 and all(bool(torch.isfinite(v).all()) for v in losses)
    c = seen[0]
    assert c['kw'] == dict(beta=1.0 / 9.0, gamma=2.0, alpha=0.25, w_cls=2.0, w_bbox=0.5)
    npos, nneg = c['counts']
    assert npos >= 1 and nneg > npos and int((c['label_w'] > 0).sum()) == npos + nneg          # every assigned anchor, no sampled subset
    ref, bound = R.rpn_focal_statement(c['o'], c['A'], c['labels'], c['label_w'], c['bbox_t'], c['bbox_w'], c['counts'], **c['kw'])
    rpn = torch.stack([got['loss_rpn_cls'][0], got['loss_rpn_bbox'][0]]).detach()
    print('loss_rpn_cls %.6g loss_rpn_bbox %.6g over %d positives, %d negatives' % (float(rpn[0]), float(rpn[1]), npos, nneg))
    check('e2e.rpn', torch.float32, rpn, ref['out2'], bound['out2'])
    assert float(rpn[0]) > 0 and float(rpn[1]) > 0
    sum(v.sum() for v in losses).backward()
    for name in ('rpn_conv', 'rpn_cls', 'rpn_reg'):
        gw = getattr(model.rpn_head, name).weight.grad
        assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0, name
    again = step()
    for k in ('loss_rpn_cls', 'loss_rpn_bbox'):
        assert torch.equal(got[k][0], again[k][0]), k
