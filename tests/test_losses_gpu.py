"""The regression / IoU / GHM loss kernels (hvrnet_amd/csrc/reg_loss.hip, ghm.hip) against the f64 statements of tests/loss_refs.py,
through native.*, the autograd ops, the loss modules and one SelsaRCNN training iteration with BalancedL1Loss in both heads.

Every bound is the derived one of loss_refs (nothing is measured against the device), every element of every output is compared.  Each
comparison prints `RATIO <what> <worst error / bound>` (pytest -s shows it)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import losses, native, ops, synthetic as S  # noqa: E402
from tests import loss_refs as R  # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = dict(smooth_l1=dict(beta=1.0 / 9.0), balanced_l1=dict(beta=1.0, alpha=0.5, gamma=1.5), mse=dict())
BOX = dict(iou=dict(eps=1e-6), bounded_iou=dict(beta=0.2, eps=1e-3))
REG_SHAPES = [(1, 4, 4), (5, 3, 3), (64, 4, 4), (257, 4, 13), (4099, 3, 3)]       # (N, D, row pitch of pred)
BOX_SIZES = [1, 7, 257, 4099]


def check(what, got, q):
    """Every element of `got` inside the bound of the statement `q`; prints the worst error / bound."""
    err = (got.double().cpu() - q.v).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / R.bound(q))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %.4g' % (what, worst))
    assert bool(torch.isfinite(got.double()).all()), what
    assert worst <= 1.0, '%s: %d of %d elements over the bound, worst error / bound %g' % (what, int((ratio > 1).sum()), ratio.numel(), worst)


def pitched(x, ld):
    """x [N, D] on the device as a view of a [N, ld] buffer."""
    buf = torch.full((x.shape[0], ld), 7.5, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]]


def smallest_partly_filled(splits, restated, cols):
    """The smallest row count for which `splits` cuts at least 3 workgroups and the last one holds fewer rows than the others."""
    for N in range(1, 100000):
        S_, rows = restated(N, cols)
        assert splits(N) == S_
        if S_ >= 3 and N % rows:
            return N
    raise AssertionError('no such shape')


def avg_forms(value):
    """(kwargs of the native call, the divisor the statement takes): a host float, a device count, and a device count of 0 (clamped to 1)."""
    return [(dict(avg=float(value)), float(value)), (dict(counts=torch.tensor([int(value)], dtype=torch.int32, device=DEV)), float(int(value))),
            (dict(counts=torch.zeros(1, dtype=torch.int32, device=DEV)), 1.0)]


# ------------------------------------------------------------------------------------------------ elementwise family
@pytest.mark.parametrize('rule', list(REG))
def test_elementwise_rules_against_f64(rule):
    prm = REG[rule]
    from tests.focal_refs import focal_loss_splits
    shapes = REG_SHAPES + [(smallest_partly_filled(lambda n: native.reg_loss_splits(n, 3), focal_loss_splits, 3), 3, 3)]
    for N, D, ld in shapes:
        pred, target, w = R.reg_case(N, D, seed=N + D, beta=prm.get('beta', 1.0))
        p, t = pitched(pred, ld), target.to(DEV)
        l, g = R.reg_elem(rule, pred, target, prm)
        tag = '%s.%dx%d@%d' % (rule, N, D, ld)
        check(tag + '.fwd', native.reg_loss_fwd(rule, p, t, **prm), l)
        dl = (0.5 + torch.rand((N, D), generator=torch.Generator().manual_seed(N))).to(DEV)
        check(tag + '.bwd', native.reg_loss_bwd(rule, p, t, dl, **prm), R.Q(dl.cpu().double()) * g)
        for wi, wt in enumerate((None, w, torch.zeros_like(w))):
            for kw, avg in avg_forms(7.0):
                out, d = native.reg_loss(rule, p, t, None if wt is None else wt.to(DEV), loss_weight=2.0, **kw, **prm)
                ro, rd = R.reg_reduced(rule, pred, target, wt, prm, 2.0, avg, ldp=ld)
                check('%s.reduced.w%d.out' % (tag, wi), out[0], ro)
                check('%s.reduced.w%d.grad' % (tag, wi), d, rd)
                out2, d2 = native.reg_loss(rule, p, t, None if wt is None else wt.to(DEV), loss_weight=2.0, **kw, **prm)
                assert torch.equal(out, out2) and torch.equal(d, d2)
            if wi == 2:
                assert float(out[0]) == 0.0 and bool((d == 0).all())      # all-zero weights: exactly 0 through the sum itself


# ------------------------------------------------------------------------------------------------ box-pair family
@pytest.mark.parametrize('aligned', [True, False], ids=['16B', 'scalar'])
@pytest.mark.parametrize('rule', list(BOX))
def test_box_pair_rules_against_f64(rule, aligned):
    prm = BOX[rule]
    from tests.focal_refs import focal_loss_splits
    sizes = BOX_SIZES + [smallest_partly_filled(native.box_loss_splits, focal_loss_splits, 4)]

    def dev(x):       # aligned: torch's own allocation; otherwise a view one float into a buffer (the scalar loads and stores)
        if aligned:
            return x.to(DEV).contiguous()
        buf = torch.zeros(x.numel() + 1, device=DEV)
        buf[1:] = x.to(DEV).reshape(-1)
        return buf[1:].view(x.shape)

    for n in sizes:
        pred, target, w_row, w_elem = R.box_case(n, seed=n)
        w = w_row if rule == 'iou' else w_elem
        p, t = dev(pred), dev(target)
        l, g = R.box_forms(rule, pred, target, prm)
        tag = '%s.%d' % (rule, n)
        check(tag + '.fwd', native.box_loss_fwd(rule, p, t, **prm), l)
        dl = (0.5 + torch.rand(tuple(l.v.shape), generator=torch.Generator().manual_seed(n)))
        _, gb = R.box_forms(rule, pred, target, prm, coef=R.Q(dl.double()))
        check(tag + '.bwd', native.box_loss_bwd(rule, p, t, dev(dl), **prm), gb)
        for wi, wt in enumerate((None, w, torch.zeros_like(w))):
            for kw, avg in avg_forms(11.0):
                out, d = native.box_loss(rule, p, t, None if wt is None else dev(wt), loss_weight=1.5, **kw, **prm)
                ro, rd = R.box_reduced(rule, pred, target, wt, prm, 1.5, avg)
                check('%s.reduced.w%d.out' % (tag, wi), out[0], ro)
                check('%s.reduced.w%d.grad' % (tag, wi), d, rd)
                out2, d2 = native.box_loss(rule, p, t, None if wt is None else dev(wt), loss_weight=1.5, **kw, **prm)
                assert torch.equal(out, out2) and torch.equal(d, d2)
            if wi == 2:
                assert float(out[0]) == 0.0 and bool((d == 0).all())


# ------------------------------------------------------------------------------------------------ GHM
def run_ghm(kind, c, momentum, acc, loss_weight, mu=0.02, labels=False):
    dev = {k: v.to(DEV) for k, v in c.items()}
    if kind == 'ghmc':
        tgt, wt = (dev['labels'], dev['label_weight']) if labels else (dev['target'], dev['weight'])
        out, d, ws = native.ghmc_loss(dev['pred'], tgt, wt, dev['edges'], momentum, acc, loss_weight)
    else:
        out, d, ws = native.ghmr_loss(dev['pred'], dev['target'], dev['weight'], dev['edges'], mu, momentum, acc, loss_weight)
    return out, d, native.ghm_workspace_views(ws, c['edges'].numel() - 1)


def check_ghm(tag, kind, c, momentum, acc0, loss_weight, mu=0.02, labels=False):
    acc = None if acc0 is None else acc0.clone().to(DEV)
    out, d, (counts, w, tot, n) = run_ghm(kind, c, momentum, acc, loss_weight, mu, labels)
    s = R.ghm_statement(kind, c['pred'], c['target'], c['weight'], c['edges'], momentum, acc0, loss_weight, mu)
    assert counts.cpu().tolist() == s['counts'].tolist(), tag
    assert int(n) == s['n'] and float(tot) == float(s['tot'].v), (tag, int(n), s['n'], float(tot), float(s['tot'].v))
    check(tag + '.out', out[0], s['out1'])
    check(tag + '.grad', d, s['d'])
    check(tag + '.w', w, s['w'])
    if momentum > 0:
        check(tag + '.acc_sum', acc, s['acc'])
    return out, d, acc, s


@pytest.mark.parametrize('kind', ['ghmc', 'ghmr'])
def test_ghm_against_f64(kind):
    Np = None       # the smallest N at 3 columns that the split cuts into >= 3 workgroups with a partly filled last one
    for N in range(1, 100000):
        S_, per = R.ghm_splits(N, 3)
        assert native.ghm_splits(N, 3) == S_
        if S_ >= 3 and (N * 3) % per:
            Np = N
            break
    for bins in (1, 10, 30, 64):
        for shape, (N, C) in (('spread', (37, 5)), ('one_bin', (64, 4)), ('gaps', (Np, 3)), ('invalid', (5, 3))):
            c = R.ghm_case(kind, N, C, bins, seed=bins + N, shape=shape)
            acc0 = torch.rand(bins, generator=torch.Generator().manual_seed(bins)) * 3
            for momentum in (0.0, 0.75):
                tag = '%s.%s.b%d.m%g' % (kind, shape, bins, momentum)
                out, d, acc, s = check_ghm(tag, kind, c, momentum, acc0 if momentum > 0 else None, 1.5)
                if shape == 'invalid':       # n = 0: loss and gradient exactly 0, acc_sum untouched
                    assert s['n'] == 0 and float(out[0]) == 0.0 and bool((d == 0).all())
                    assert momentum == 0 or torch.equal(acc.cpu(), acc0)
                if shape == 'one_bin' and bins in (1, 10):
                    assert s['n'] == 1
                if shape == 'gaps' and bins >= 10:
                    assert 1 < s['n'] < bins
    if kind == 'ghmc':       # the labels form: _expand_binary_labels on the device
        c = R.ghm_case('ghmc', 37, 5, 10, seed=77, labels=True)
        check_ghm('ghmc.labels', 'ghmc', c, 0.0, None, 1.0, labels=True)


@pytest.mark.parametrize('run', ['ghmc_m75', 'ghmr_m75', 'ghmc_m0'])
def test_ghm_modules_follow_the_reference_over_three_calls(run):
    """Three consecutive calls on one module against the reference's own losses, gradients and acc_sum trail (tests/golden/losses.npz).
    The golden numbers are f64; the tolerance is the statement's bound around the statement, which the CPU suite ties to the golden at
    1e-10, plus that 1e-10."""
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(ROOT, 'tests', 'golden', 'losses.npz')).items()}
    kind, bins, momentum, loss_weight, by_label = R.GHM_RUNS[run]
    mu = float(g[run + '.cfg'][3])
    m = (losses.GHMC(bins=bins, momentum=momentum, loss_weight=loss_weight) if kind == 'ghmc'
         else losses.GHMR(mu=mu, bins=bins, momentum=momentum, loss_weight=loss_weight)).to(DEV)
    acc = torch.zeros(bins)
    for i in range(3):
        p = '%s.%d.' % (run, i)
        pred, target, weight = g[p + 'pred'], g[p + 'target'], g[p + 'weight']
        x = pred.to(DEV).requires_grad_(True)
        loss = m(x, target.to(DEV), weight.to(DEV))
        loss.backward()
        td, wd = R.expand_binary_labels(target, weight, pred.shape[1]) if by_label else (target, weight)
        s = R.ghm_statement(kind, pred, td, wd, g[run + '.edges'], momentum, acc, loss_weight, mu)
        for what, got, q, gold in (('loss', loss.detach(), s['out1'], g[p + 'loss']), ('grad', x.grad, s['d'], g[p + 'grad'])):
            check('%s.%d.%s' % (run, i, what), got, q)
            assert bool(((got.double().cpu() - gold.double()).abs() <= R.bound(q) + 1e-10 * gold.abs().max()).all()), (run, i, what)
        if momentum > 0:
            check('%s.%d.acc_sum' % (run, i), m.acc_sum, s['acc'])
            assert bool(((m.acc_sum.double().cpu() - g[p + 'acc_sum']).abs() <= R.bound(s['acc']) + 1e-10 * g[p + 'acc_sum'].abs().max()).all())
            acc = m.acc_sum.detach().cpu().clone()          # the next call starts from the module's own f32 buffer


# ------------------------------------------------------------------------------------------------ graphs
def test_graph_replay_equals_eager_and_advances_acc_sum_once():
    pred, target, w = R.reg_case(257, 4, seed=5)
    p, t, wd = pred.to(DEV), target.to(DEV), w.to(DEV)
    bp, bt, bw, _ = R.box_case(257, seed=6)
    bp, bt, bw = bp.to(DEV), bt.to(DEV), bw.to(DEV)
    c = {k: v.to(DEV) for k, v in R.ghm_case('ghmc', 257, 4, 10, seed=7).items()}
    counts = torch.tensor([9], dtype=torch.int32, device=DEV)
    acc = torch.ones(10, device=DEV)

    def calls():
        a = native.reg_loss('balanced_l1', p, t, wd, loss_weight=2.0, counts=counts, **REG['balanced_l1'])
        b = native.box_loss('iou', bp, bt, bw, loss_weight=1.0, avg=3.0, **BOX['iou'])
        e = native.box_loss_fwd('bounded_iou', bp, bt, **BOX['bounded_iou'])
        g = native.ghmc_loss(c['pred'], c['target'], c['weight'], c['edges'], 0.75, acc, 1.0)
        return a + b + (e,) + g[:2]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    acc.fill_(1.0)
    eager = [x.clone() for x in calls()]
    acc_after_one = acc.clone()
    acc.fill_(1.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = calls()
    acc.fill_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    assert torch.equal(acc, acc_after_one)          # one replay, one momentum step
    graph.replay()
    torch.cuda.synchronize()
    s = R.ghm_statement('ghmc', c['pred'].cpu(), c['target'].cpu(), c['weight'].cpu(), c['edges'].cpu(), 0.75, acc_after_one.cpu(), 1.0)
    check('graph.acc_sum.second_replay', acc, s['acc'])
    assert not torch.equal(acc, acc_after_one)


# ------------------------------------------------------------------------------------------------ autograd and modules
def test_modules_equal_the_native_calls_and_backward_works():
    pred, target, w = R.reg_case(64, 4, seed=21)
    bp, bt, w_row, w_elem = R.box_case(64, seed=22)
    cases = [(losses.SmoothL1Loss, 'smooth_l1', dict(beta=1.0 / 9.0), pred, target, w), (losses.BalancedL1Loss, 'balanced_l1', REG['balanced_l1'], pred, target, w),
             (losses.MSELoss, 'mse', dict(), pred, target, w), (losses.IoULoss, 'iou', BOX['iou'], bp, bt, w_row),
             (losses.BoundedIoULoss, 'bounded_iou', BOX['bounded_iou'], bp, bt, w_elem)]
    for cls, rule, prm, a, b, wt in cases:
        reg = rule in REG
        fused = native.reg_loss if reg else native.box_loss
        fwd = native.reg_loss_fwd if reg else native.box_loss_fwd
        a_d, b_d, w_d = a.to(DEV), b.to(DEV), wt.to(DEV)
        count = float(a.numel() if rule != 'iou' else a.shape[0])
        for red, avg_factor, avg in (('mean', 11.0, 11.0), ('mean', None, count), ('sum', None, 1.0)):
            m = cls(reduction=red, loss_weight=2.0, **prm)
            x = a_d.clone().requires_grad_(True)
            out = m(x, b_d, w_d, avg_factor=avg_factor)
            (out * 3.0).backward()
            o1, d1 = fused(rule, a_d, b_d, w_d, loss_weight=2.0, avg=avg, **prm)
            assert torch.equal(out.detach(), o1[0]) and torch.equal(x.grad, d1 * 3.0), (rule, red)
        m = cls(loss_weight=2.0, **prm)
        x = a_d.clone().requires_grad_(True)
        none = m(x, b_d, w_d, reduction_override='none')
        assert torch.equal(none.detach(), 2.0 * (fwd(rule, a_d, b_d, **prm) * w_d))
        none.sum().backward()
        rule_fn = dict(smooth_l1=ops.smooth_l1_loss, balanced_l1=ops.balanced_l1_loss, mse=ops.mse_loss, iou=ops.iou_loss, bounded_iou=ops.bounded_iou_loss)[rule]
        x2 = a_d.clone().requires_grad_(True)
        (rule_fn(x2, b_d, **prm) * w_d * 2.0).sum().backward()
        assert torch.equal(x.grad, x2.grad) and float(x.grad.abs().max()) > 0, rule
        dev_avg = m(a_d, b_d, w_d, avg_factor=torch.tensor([11], dtype=torch.int32, device=DEV))
        assert torch.equal(dev_avg, m(a_d, b_d, w_d, avg_factor=11.0)), rule
    with pytest.raises(native.HvrError, match='ws_bytes|workspace'):
        native.reg_loss('mse', pred.to(DEV), target.to(DEV), ws=torch.zeros(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(native.HvrError, match='bins'):
        native.ghmr_loss(pred.to(DEV), target.to(DEV), w.to(DEV), torch.linspace(0, 1, 67, device=DEV))


# ------------------------------------------------------------------------------------------------ end to end
def _selsa(loss_type, form, ohem=False):
    from hvrnet_amd.config import selsa_train_config
    cfg = selsa_train_config(nms_post=8, rcnn_sampler_num=4, t_dim=3, ohem=ohem)
    cfg.model.backbone['depth'] = 50
    cfg.model.shared_head['depth'] = 50
    box = dict(type=loss_type, beta=1.0, loss_weight=1.0)
    cfg.model.rpn_head.update(anchor_scales=[1, 1.5, 2, 4], loss_bbox=dict(box))
    if form == 'focal':
        cfg.model.rpn_head.update(loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0))
    cfg.model.bbox_head.update(loss_bbox=dict(box))
    return hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, S.synth_state_dict('selsa', depth=50), torch.float32, DEV))


@pytest.mark.parametrize('form', ['bce', 'focal'])
def test_selsa_trains_with_balanced_l1_in_both_heads(monkeypatch, form):
    """One SelsaRCNN iteration with loss_bbox type BalancedL1Loss in rpn_head and bbox_head: the box terms equal the statement on the
    inputs the module was handed, the classification terms and acc are the bits of the same model under SmoothL1Loss, gradients reach the
    RPN and head weights, a second call gives the same bits."""
    Tn, hw = 3, (64, 64)
    g = torch.Generator().manual_seed(91)
    imgs = (torch.randn((Tn, 3) + hw, generator=g) * 50.0).to(DEV)
    metas = [dict(img_shape=hw + (3,), pad_shape=hw + (3,), scale_factor=1.0, flip=False) for _ in range(Tn)]
    gt_b = torch.tensor([[8., 8., 39., 39.], [30., 20., 60., 50.]]).to(DEV)
    gt_l = torch.tensor([5, 12]).to(DEV)
    keys = dict(rcnn=[torch.rand(2 + 8, generator=g).to(DEV) for _ in range(Tn)], rpn=torch.rand(4 * 4 * 12, generator=g).to(DEV))
    seen = []
    real = losses.BalancedL1Loss.forward

    def spy(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        avg = float(max(int(avg_factor[0]), 1)) if torch.is_tensor(avg_factor) else float(avg_factor)
        seen.append(dict(pred=pred.detach().cpu().clone(), target=target.cpu().clone(), w=weight.cpu().clone(), avg=avg, ldp=pred.stride(0)))
        return real(self, pred, target, weight, avg_factor, reduction_override)

    monkeypatch.setattr(losses.BalancedL1Loss, 'forward', spy)

    def step(model):
        return model(imgs, metas, return_loss=True, gt_bboxes=[gt_b] * Tn, gt_labels=[gt_l] * Tn, keys=keys)

    model = _selsa('BalancedL1Loss', form)
    got = step(model)
    assert len(seen) == 2
    prm = dict(beta=1.0, alpha=0.5, gamma=1.5)
    for c, term in zip(seen, (got['loss_rpn_bbox'][0], got['loss_bbox'])):
        ref, _ = R.reg_reduced('balanced_l1', c['pred'], c['target'], c['w'], prm, 1.0, c['avg'], ldp=c['ldp'])
        check('e2e.%s.box_term' % form, term.detach(), ref)
        assert int((c['w'] > 0).sum()) > 0 and float(term) > 0
    assert seen[1]['avg'] == float(seen[1]['target'].shape[0])           # BBoxHead.loss: avg_factor = bbox_targets.size(0)
    losses_ = [v if isinstance(v, torch.Tensor) else sum(v) for k, v in got.items() if 'loss' in k]
    sum(v.sum() for v in losses_).backward()
    for mod in (model.rpn_head.rpn_conv, model.rpn_head.rpn_reg, model.rpn_head.rpn_cls, model.bbox_head.fc_reg, model.bbox_head.fc_cls):
        gw = mod.weight.grad
        assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    again = step(model)
    for k in ('loss_rpn_cls', 'loss_rpn_bbox'):
        assert torch.equal(got[k][0], again[k][0]), k
    for k in ('loss_cls', 'loss_bbox', 'acc'):
        assert torch.equal(got[k], again[k]), k
    smooth = step(_selsa('SmoothL1Loss', form))
    assert torch.equal(got['loss_rpn_cls'][0], smooth['loss_rpn_cls'][0])
    assert torch.equal(got['loss_cls'], smooth['loss_cls']) and torch.equal(got['acc'], smooth['acc'])
    assert not torch.equal(got['loss_bbox'], smooth['loss_bbox'])
    # the wiring (column slice, reshape order, weights, avg_factor): the tensors the module was handed, through the smooth-L1 rule, give the
    # box terms the FUSED kernels of the SmoothL1Loss model compute from the same head outputs.  Those kernels add the same terms in another
    # order and scale by `/ avg * w` instead of `* (w / avg)`: the chain counted is the number of terms, which bounds every order, and four
    # more roundings stand for the other scaling.
    for c, term in zip(seen, (smooth['loss_rpn_bbox'][0], smooth['loss_bbox'])):
        ref, _ = R.reg_reduced('smooth_l1', c['pred'], c['target'], c['w'], dict(beta=1.0), 1.0, c['avg'], chain=c['pred'].numel())
        check('e2e.%s.wiring' % form, term.detach(), R.Q(ref.v, ref.e + 4 * R.U * ref.v.abs()))
        assert float(term) > 0


def test_the_ohem_form_refuses_balanced_l1_by_name():
    model = _selsa('BalancedL1Loss', 'bce', ohem=True)
    imgs = torch.zeros((3, 3, 64, 64), device=DEV)
    metas = [dict(img_shape=(64, 64, 3), pad_shape=(64, 64, 3), scale_factor=1.0, flip=False)] * 3
    gt_b, gt_l = torch.tensor([[8., 8., 39., 39.]]).to(DEV), torch.tensor([5]).to(DEV)
    with pytest.raises(NotImplementedError, match="loss_bbox type 'BalancedL1Loss' is not on the HIP path of the OHEM form"):
        model(imgs, metas, return_loss=True, gt_bboxes=[gt_b] * 3, gt_labels=[gt_l] * 3)
