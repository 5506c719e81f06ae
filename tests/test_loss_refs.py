"""CPU checks of the regression / IoU / GHM loss statements (tests/loss_refs.py) and of the host side of the feature: the statements
against the reference's own numbers (tests/golden/losses.npz), the f32 emulation inside every bound, every named mistake outside one,
and the module / registry / head surface with its refusals.  No GPU."""
import os

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import losses, registry
from hvrnet_amd.losses import GHMC, GHMR, BalancedL1Loss      # the module under test: this file has nothing to check without it
from tests import loss_refs as R
from tests.loss_refs import CASES, GHM_RUNS, PRM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = dict(smooth_l1=dict(beta=1.0 / 9.0), balanced_l1=dict(beta=1.0, alpha=0.5, gamma=1.5), mse=dict())
BOX = dict(iou=dict(eps=1e-6), bounded_iou=dict(beta=0.2, eps=1e-3))
REG_SHAPES = [(1, 4), (5, 3), (64, 4), (257, 4), (4099, 3)]
BOX_SIZES = [1, 7, 257, 4099]
BAR = 1e-10      # both sides are f64 evaluations of one formula and differ in summation order only


@pytest.fixture(scope='module')
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(ROOT, 'tests', 'golden', 'losses.npz')).items()}


def close(a, b, scale):
    return bool(((a.double() - b.double()).abs() <= BAR * scale).all())


# ------------------------------------------------------------------------------------------------ statements against the golden
@pytest.mark.parametrize('rule', list(CASES))
@pytest.mark.parametrize('case', ['a', 'b'])
def test_statement_equals_the_reference(golden, rule, case):
    p = '%s.%s.' % (rule, case)
    pred, target, w, avg = golden[p + 'pred'], golden[p + 'target'], golden[p + 'w'], float(golden[p + 'avg'])
    prm = dict(zip(PRM[rule], golden[p + 'prm'].tolist()))
    if rule in BOX:
        l, _ = R.box_forms(rule, pred, target, prm)
        count = float(l.v.numel())

        def reduced(wt, lw, a):
            return R.box_reduced(rule, pred, target, wt, prm, lw, a)
    else:
        l, _ = R.reg_elem(rule, pred, target, prm)
        count = float(pred.numel())

        def reduced(wt, lw, a):
            return R.reg_reduced(rule, pred, target, wt, prm, lw, a)
    big = float(l.v.abs().max())
    assert close(reduced(None, 1.0, count)[0].v, golden[p + 'mean'], big)
    if rule == 'mse':      # the reference's mse_loss lets F.mse_loss average before weight_reduce_loss sees the elements (mse_loss.py:7): only
        # its unweighted 'mean' is the rule's (include/hvr_hip.h and DESIGN.md 8p name the departure).  'none', the weighted forms and the
        # gradient are held to the rule written out on the stored inputs in f64, with weight_reduce_loss's reductions.
        assert p + 'none' not in golden
        d64, w64 = pred.double() - target.double(), w.double()
        assert close(l.v, d64 * d64, big)
        assert close(reduced(w, 1.0, count)[0].v, (w64 * d64 * d64).sum() / count, big)
        assert close(reduced(w, 1.0, avg)[0].v, (w64 * d64 * d64).sum() / avg, big)
        out, d = reduced(w, 3.0, 1.0)
        assert close(out.v, 3.0 * (w64 * d64 * d64).sum(), 3.0 * big * count)
        assert close(d.v, 3.0 * w64 * 2.0 * d64, float((6.0 * d64).abs().max()))
        return
    assert close(l.v, golden[p + 'none'], big)
    assert close(reduced(w, 1.0, count)[0].v, golden[p + 'mean_w'], big)
    assert close(reduced(w, 1.0, avg)[0].v, golden[p + 'mean_avg'], big)
    out, d = reduced(w, 1.0, 1.0)
    assert close(out.v, golden[p + 'sum_w'], big * count)
    keep = ~golden[p + 'tie']
    g = golden[p + 'grad_sum_w']
    assert close(d.v[keep], g[keep], float(g.abs().max()))
    assert bool(keep.any())


@pytest.mark.parametrize('run', list(GHM_RUNS))
def test_ghm_statement_equals_the_reference_over_three_calls(golden, run):
    kind, bins, momentum, loss_weight, by_label = GHM_RUNS[run]
    mu = float(golden[run + '.cfg'][3])
    edges = golden[run + '.edges']
    assert bool((edges == R.ghm_edges(bins, kind)).all())
    acc = torch.zeros(bins)
    for i in range(3):
        p = '%s.%d.' % (run, i)
        pred, target, weight = golden[p + 'pred'], golden[p + 'target'], golden[p + 'weight']
        if by_label:
            target, weight = R.expand_binary_labels(target, weight, pred.shape[1])
        s = R.ghm_statement(kind, pred, target, weight, edges, momentum, acc, loss_weight, mu)
        assert close(s['out1'].v, golden[p + 'loss'], float(golden[p + 'loss'].abs()))
        assert close(s['d'].v, golden[p + 'grad'], float(golden[p + 'grad'].abs().max()))
        if momentum > 0:
            assert close(s['acc'].v, golden[p + 'acc_sum'], float(golden[p + 'acc_sum'].abs().max()))
            acc = s['acc'].v          # the f64 trail: Q takes its values exactly
        assert not bool((R._near_edge(s['g'], edges) & (weight > 0)).any())


# ------------------------------------------------------------------------------------------------ emulation inside, mistakes outside
@pytest.mark.parametrize('rule', list(REG))
def test_f32_emulation_of_the_elementwise_rules_lies_inside_the_bounds(rule):
    prm = REG[rule]
    for N, D in REG_SHAPES:
        pred, target, w = R.reg_case(N, D, seed=N + D, beta=prm.get('beta', 1.0))
        l, g = R.reg_elem(rule, pred, target, prm)
        lf, gf = R.reg_elem(rule, pred, target, prm, exact=False)
        assert R.inside(lf, l) and R.inside(gf, g), (N, D)
        for wt in (None, w, torch.zeros_like(w)):
            out, d = R.reg_reduced(rule, pred, target, wt, prm, 2.0, 7.0)
            of, df = R.reg_reduced(rule, pred, target, wt, prm, 2.0, 7.0, exact=False)
            assert R.inside(of, out) and R.inside(df, d), (N, D)
        assert float(out.v) == 0.0 and float(of) == 0.0          # all-zero weights: exactly 0 through the sum itself


@pytest.mark.parametrize('rule', list(BOX))
def test_f32_emulation_of_the_box_rules_lies_inside_the_bounds(rule):
    prm = BOX[rule]
    for n in BOX_SIZES:
        pred, target, w_row, w_elem = R.box_case(n, seed=n)
        w = w_row if rule == 'iou' else w_elem
        l, g = R.box_forms(rule, pred, target, prm)
        lf, gf = R.box_forms(rule, pred, target, prm, exact=False)
        assert bool(torch.isfinite(lf).all() and torch.isfinite(gf).all())
        assert R.inside(lf, l) and R.inside(gf, g), n
        out, d = R.box_reduced(rule, pred, target, w, prm, 1.5, 11.0)
        of, df = R.box_reduced(rule, pred, target, w, prm, 1.5, 11.0, exact=False)
        assert R.inside(of, out) and R.inside(df, d), n


def test_iou_gradient_is_zero_below_eps_and_follows_pred_on_ties():
    pred, target, _, _ = R.box_case(10, seed=3)
    l, g = R.box_forms('iou', pred, target, BOX['iou'])
    kinds = [R.BOX_KINDS[i % 5] for i in range(10)]
    for i, k in enumerate(kinds):
        if k in ('disjoint', 'degenerate'):
            assert float(l.v[i]) == pytest.approx(-np.log(np.float32(1e-6)), rel=1e-6) and bool((g.v[i] == 0).all())
        if k == 'identical':      # iou = 1, pred takes the gradient of every max / min: dI = dA, so g = 0 - dI / I = -+ 1 / side
            assert float(l.v[i]) == 0.0 and bool((g.v[i] != 0).all())


@pytest.mark.parametrize('kind', ['ghmc', 'ghmr'])
@pytest.mark.parametrize('shape', ['spread', 'one_bin', 'gaps', 'invalid'])
def test_f32_emulation_of_ghm_lies_inside_the_bounds(kind, shape):
    for bins in (1, 10, 30, 64):
        c = R.ghm_case(kind, 37, 5, bins, seed=bins, shape=shape)
        acc = torch.rand(bins, generator=torch.Generator().manual_seed(1)) * 3
        for momentum in (0.0, 0.75):
            s = R.ghm_statement(kind, c['pred'], c['target'], c['weight'], c['edges'], momentum, acc, 1.5)
            f = R.ghm_statement(kind, c['pred'], c['target'], c['weight'], c['edges'], momentum, acc, 1.5, exact=False)
            assert bool((s['counts'] == f['counts']).all()) and s['n'] == f['n']
            assert R.inside(f['out1'], s['out1']) and R.inside(f['d'], s['d']) and R.inside(f['w'], s['w']) and R.inside(f['tot'], s['tot'])
            if momentum > 0:
                assert R.inside(f['acc'], s['acc'])
            if shape == 'invalid':
                assert s['n'] == 0 and float(s['out1'].v) == 0.0 and bool((s['d'].v == 0).all()) and float(s['tot'].v) == 1.0
                assert momentum == 0 or bool((s['acc'].v == acc.double()).all())
            if shape == 'one_bin' and bins in (1, 10):
                assert s['n'] == 1
            if shape == 'gaps' and bins >= 10:
                assert 1 < s['n'] < bins


def _outside(got, q):
    return not R.inside(got, q)


@pytest.mark.parametrize('rule,mistake', [(r, m) for r in ('balanced_l1', 'iou', 'bounded_iou') for m in R.MISTAKES[r]])
def test_every_named_mistake_of_the_rules_lands_outside_a_bound(rule, mistake):
    hit = False
    if rule == 'balanced_l1':
        pred, target, w = R.reg_case(64, 4, seed=8)
        l, g = R.reg_elem(rule, pred, target, REG[rule])
        lm, gm = R.reg_elem(rule, pred, target, REG[rule], mistake=mistake)
        out = R.reg_reduced(rule, pred, target, w, REG[rule], 1.0, 64.0)[0]
        outm = R.reg_reduced(rule, pred, target, w, REG[rule], 1.0, 64.0, mistake=mistake)[0]
        hit = _outside(lm.v, l) and _outside(outm.v, out)
    else:
        pred, target, w_row, w_elem = R.box_case(20, seed=8)
        w = w_row if rule == 'iou' else w_elem
        l, g = R.box_forms(rule, pred, target, BOX[rule])
        lm, gm = R.box_forms(rule, pred, target, BOX[rule], mistake=mistake)
        out = R.box_reduced(rule, pred, target, w, BOX[rule], 1.0, 20.0)[0]
        outm = R.box_reduced(rule, pred, target, w, BOX[rule], 1.0, 20.0, mistake=mistake)[0]
        hit = _outside(lm.v, l) and _outside(outm.v, out)
    assert hit


@pytest.mark.parametrize('kind,mistake', [(k, m) for k in ('ghmc', 'ghmr') for m in R.MISTAKES[k]])
def test_every_named_mistake_of_ghm_lands_outside_a_bound(kind, mistake):
    if mistake in ('right_closed_bins', 'last_edge_at_one'):
        c = R.ghmc_edge_case()
    else:
        c = R.ghm_case(kind, 37, 5, 10, seed=4, shape='gaps')
    acc = torch.arange(1, 11).float()
    s = R.ghm_statement(kind, c['pred'], c['target'], c['weight'], c['edges'], 0.75, acc, 1.0)
    m = R.ghm_statement(kind, c['pred'], c['target'], c['weight'], c['edges'], 0.75, acc, 1.0, mistake=mistake)
    # (tot cancels between the bin weights and the division of the loss: a wrong tot shows in `tot` and `w`, which the workspace keeps)
    differs = [_outside(m[k].v, s[k]) for k in ('out1', 'd', 'acc', 'tot', 'w')] + [not bool((m['counts'] == s['counts']).all()), m['n'] != s['n']]
    assert any(differs), differs


def test_the_ghm_case_generator_keeps_its_margin():
    for kind in ('ghmc', 'ghmr'):
        for bins in (1, 10, 30, 64):
            c = R.ghm_case(kind, 257, 7, bins, seed=bins + 1)
            g = R.val(R._ghm_g(kind, c['pred'], c['target'], 0.02, True)[0])
            assert not bool((R._near_edge(g, c['edges']) & (c['weight'] > 0)).any())
    e = R.ghmc_edge_case()
    g = R.val(R._ghm_g('ghmc', e['pred'], e['target'], 0.02, True)[0])
    assert bool(R._near_edge(g, e['edges']).any())      # the hand-made case sits on edges on purpose


def test_split_restatements_cut_into_non_empty_workgroups():
    for N, C in ((1, 1), (5, 3), (2049, 4), (4099, 3), (150000, 80)):
        S, per = R.ghm_splits(N, C)
        assert (S - 1) * per < N * C <= S * per


# ------------------------------------------------------------------------------------------------ modules, registry, heads
NAMES = ('SmoothL1Loss', 'BalancedL1Loss', 'MSELoss', 'IoULoss', 'BoundedIoULoss', 'GHMC', 'GHMR')


def test_registry_builds_every_loss_of_the_reference_package():
    for name in NAMES:
        m = registry.build_loss(dict(type=name))
        assert type(m).__name__ == name and getattr(hvrnet_amd, name) is type(m)
    m = registry.build_loss(dict(type='BalancedL1Loss', alpha=0.75, gamma=2.0, beta=0.5, reduction='sum', loss_weight=3.0))
    assert (m.alpha, m.gamma, m.beta, m.reduction, m.loss_weight) == (0.75, 2.0, 0.5, 'sum', 3.0)
    m = registry.build_loss(dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))      # the default of every head in the reference
    assert m.beta == 1.0 / 9.0
    assert registry.build_loss(dict(type='IoULoss')).eps == 1e-6 and registry.build_loss(dict(type='BoundedIoULoss')).beta == 0.2


def test_ghm_buffers_carry_the_reference_names():
    m = GHMC(bins=10, momentum=0.75)
    assert sorted(m.state_dict()) == ['acc_sum', 'edges']
    assert bool((m.edges == R.ghm_edges(10, 'ghmc')).all()) and bool((m.acc_sum == 0).all())
    assert sorted(GHMC(bins=30).state_dict()) == ['edges']
    r = GHMR(mu=0.02, bins=10, momentum=0.5)
    assert sorted(r.state_dict()) == ['acc_sum', 'edges'] and float(r.edges[-1]) == 1000.0
    m2 = GHMC(bins=10, momentum=0.75)
    m2.load_state_dict({'edges': m.edges.clone(), 'acc_sum': torch.arange(10).float()})
    assert float(m2.acc_sum[3]) == 3.0


def test_constructor_and_argument_validation():
    with pytest.raises(NotImplementedError):
        GHMC(use_sigmoid=False)
    with pytest.raises(AssertionError, match='bins'):
        GHMC(bins=65)
    with pytest.raises(AssertionError):
        losses.SmoothL1Loss(beta=0.0)
    x, t = torch.zeros(3, 4), torch.zeros(3, 4)
    for name in NAMES[:5]:
        m = registry.build_loss(dict(type=name))
        with pytest.raises(NotImplementedError, match='%s runs on the GPU only' % name):
            m(x, t)
        with pytest.raises(ValueError, match='avg_factor can not be used with reduction="sum"'):
            m(x, t, avg_factor=2.0, reduction_override='sum')
        with pytest.raises(AssertionError):
            m(x, t, reduction_override='median')
    with pytest.raises(NotImplementedError, match='GHMC runs on the GPU only'):
        GHMC()(x, t, torch.ones(3, 4))
    with pytest.raises(NotImplementedError, match='GHMR runs on the GPU only'):
        GHMR()(x, t, torch.ones(3, 4), avg_factor=5.0)


def test_heads_read_the_loss_bbox_type():
    for typ in ('SmoothL1Loss', 'BalancedL1Loss'):
        h = hvrnet_amd.RPNHead(16, feat_channels=16, anchor_strides=[16], loss_bbox=dict(type=typ, beta=1.0 / 9.0, loss_weight=1.0))
        assert h.loss_bbox_type == typ
        b = hvrnet_amd.BBoxHead(reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5, loss_bbox=dict(type=typ, beta=1.0))
        assert b.loss_bbox_type == typ
    assert isinstance(h.loss_bbox, BalancedL1Loss) and isinstance(b.loss_bbox, BalancedL1Loss)
    with pytest.raises(NotImplementedError, match="RPNHead: loss_bbox type 'IoULoss'"):
        hvrnet_amd.RPNHead(16, feat_channels=16, anchor_strides=[16], loss_bbox=dict(type='IoULoss'))
    with pytest.raises(NotImplementedError, match="BBoxHead: loss_bbox type 'IoULoss'"):
        hvrnet_amd.BBoxHead(reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5, loss_bbox=dict(type='IoULoss'))
    with pytest.raises(NotImplementedError, match="loss_bbox type 'GHMR'"):
        hvrnet_amd.SelsaBBoxHead(4, 3, reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5, loss_bbox=dict(type='GHMR'))


def _hvr_head(loss_type):
    return hvrnet_amd.HRNMPBBoxHead(4, 3, 3, reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5, fc_feat_dim=16, dim=(16, 16, 16),
                                    loss_bbox=dict(type=loss_type, beta=1.0))


def test_hrnmp_head_refuses_balanced_l1_in_loss_and_loss_train():
    """HRNMPBBoxHead.loss / loss_train name the box loss they cannot run on their first line: CPU tensors never reach a kernel."""
    head = _hvr_head('BalancedL1Loss')
    assert head.loss_bbox_type == 'BalancedL1Loss'
    logits = [torch.zeros(6, 9), torch.zeros(6, 9)]
    lab, lw, bt, bw = torch.zeros(6, dtype=torch.long), torch.ones(6), torch.zeros(6, 4), torch.zeros(6, 4)
    msg = "HRNMPBBoxHead: loss_bbox type 'BalancedL1Loss' is not on the HIP path of HRNMPBBoxHead.loss"
    with pytest.raises(NotImplementedError, match=msg):
        head.loss_train(logits, lab, lw, bt, bw)
    with pytest.raises(NotImplementedError, match=msg):
        head.loss([x[:, :5] for x in logits], [x[:, 5:] for x in logits], lab, lw, bt, bw)
    with pytest.raises(NotImplementedError) as e:      # under SmoothL1Loss the same call passes the guard and stops at the GPU-only kernel
        _hvr_head('SmoothL1Loss').loss_train(logits, lab, lw, bt, bw)
    assert 'BalancedL1Loss' not in str(e.value)


def test_hnmb_rcnn_refuses_balanced_l1_before_anything_is_launched():
    """HNMBRCNN.forward_train with bbox_head.loss_bbox type BalancedL1Loss raises the head's message on CPU tensors: the refusal stands
    ahead of the backbone, which would raise the GPU-only error first if anything were launched before it."""
    from hvrnet_amd.config import hvr_train_config
    cfg = hvr_train_config()
    cfg.model.bbox_head.update(loss_bbox=dict(type='BalancedL1Loss', beta=1.0, loss_weight=1.0))
    model = hvrnet_amd.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    imgs = torch.zeros((15, 3, 32, 32))
    metas = [dict(img_shape=(32, 32, 3), pad_shape=(32, 32, 3), scale_factor=1.0, flip=False)] * 15
    gt_b, gt_l = [torch.tensor([[2., 2., 20., 20.]])] * 15, [torch.tensor([3])] * 15
    with pytest.raises(NotImplementedError, match="loss_bbox type 'BalancedL1Loss' is not on the HIP path of HRNMPBBoxHead.loss"):
        model.forward_train(imgs, metas, gt_b, gt_l)
    cfg.model.bbox_head.update(loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    smooth = hvrnet_amd.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    with pytest.raises(NotImplementedError) as e:      # the same call under SmoothL1Loss gets as far as the first kernel
        smooth.forward_train(imgs, metas, gt_b, gt_l)
    assert 'BalancedL1Loss' not in str(e.value)


def test_the_fused_paths_refuse_balanced_l1_by_name():
    b = hvrnet_amd.BBoxHead(reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5, loss_bbox=dict(type='BalancedL1Loss'))
    with pytest.raises(NotImplementedError, match="loss_bbox type 'BalancedL1Loss' is not on the HIP path of the OHEM form"):
        b.refuse_balanced_l1('the OHEM form')
    hvrnet_amd.BBoxHead(reg_class_agnostic=True, in_channels=8, roi_feat_size=1, num_classes=5).refuse_balanced_l1('anything')      # SmoothL1Loss passes
