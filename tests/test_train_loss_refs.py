"""The f64 statements and bounds of tests/train_loss_refs.py checked on the host, without a GPU:
  * every statement against torch's own operators in f64 (1e-12 relative) and against the loss values recorded from the
    reference's modules in g11_selsa_train.npz / g12_targets.npz (the tolerances those fixtures' own tests use);
  * not too tight: on every input set the GPU tests use, the same statement evaluated by plain PyTorch in f32 (a second,
    independent order of operations) lies within the bound of the f64 reference;
  * not too loose: plausible kernel mistakes applied to the reference move it by at least ten times the bound on those inputs.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_loss_refs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def gold(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def close(a, b, rtol, atol):
    torch.testing.assert_close(torch.as_tensor(np.asarray(a)).float().reshape(-1), torch.as_tensor(np.asarray(b)).float().reshape(-1),
                               rtol=rtol, atol=atol)


def rel12(a, b, floor=0.0):
    """1e-12 relative; `floor`: the magnitude of the operands where the quantity is a difference of much larger f64 numbers (a row's
    cross entropy is lse - x_label: both sides carry 2^-53 of max|x|, whatever is left after the cancellation)."""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    tol = 1e-12 * b.abs() + 8 * 2.0 ** -53 * torch.as_tensor(floor, dtype=torch.float64) + 1e-300
    assert bool(((a - b).abs() <= tol).all()), float(((a - b).abs() / tol).max())


def inside(got, ref, bound, what=''):
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), '%s: worst error / bound %g' % (what, float((err / bound.clamp(min=1e-300)).max()))


def moved_tenfold(wrong, ref, bound):
    """True where a mistaken result is non-finite or differs from the reference by at least ten times the bound."""
    diff = (wrong - ref).abs()
    return ~torch.isfinite(wrong) | (diff >= 10 * bound)


DET = L.det_params()


def _det_args(case, sel):
    return dict(logits=case['logits'], cls_off=case['cls_off'], reg_off=case['reg_off'], ncls=case['ncls'], labels=case['labels'],
                label_w=case['label_w'], bbox_t=case['bbox_t'], bbox_w=case['bbox_w'], beta=case['beta'], sel_counts=sel)


# ------------------------------------------------------------------------------------------------ det loss / ce rows
@pytest.mark.parametrize('name,p', [d for d in DET if d[1]['R'] in (257, 4500)], ids=lambda v: v if isinstance(v, str) else '')
def test_det_statement_equals_torch_in_f64(name, p):
    """cross entropy, smooth-L1 (scaled for beta) and their autograd gradient from torch.nn.functional in f64."""
    case, sel = L.det_build(p)
    ref, _ = L.det_loss_statement(**_det_args(case, sel))
    R, co, ro, nc = p['R'], case['cls_off'], case['reg_off'], case['ncls']
    beta = L.f32v(case['beta'])
    lg = case['logits'].double().requires_grad_(True)
    avg = max(float((case['label_w'] > 0).sum()), 1.0)
    rows = float(max(sum(sel), 1)) if sel is not None else float(R)
    lc = (F.cross_entropy(lg[:, co:co + nc], case['labels'], reduction='none') * case['label_w'].double()).sum() / avg
    pos = (case['labels'] > 0).double()[:, None]
    l1 = F.smooth_l1_loss(lg[:, ro:ro + 4] / beta, case['bbox_t'].double() / beta, reduction='none') * beta
    lb = (l1 * case['bbox_w'].double() * pos).sum() / rows
    (lc + lb).backward()
    rel12(ref['out3'][0], lc.detach())
    rel12(ref['out3'][1], lb.detach())
    # (torch's smooth-L1 is given pred / beta and target / beta: each carries 2^-53 of its own size into a difference that may be
    # far smaller, hence the floor relative to the largest gradient)
    assert torch.allclose(ref['dlogits'], lg.grad, rtol=1e-12, atol=1e-13 * float(lg.grad.abs().max()))
    live = torch.zeros(case['logits'].shape[1], dtype=torch.bool)
    live[co:co + nc] = True
    live[ro:ro + 4] = True
    assert bool((ref['dlogits'][:, ~live] == 0).all())
    ce, _ = L.ce_rows_statement(case['logits'], co, nc, case['labels'])
    rel12(ce, F.cross_entropy(case['logits'].double()[:, co:co + nc], case['labels'], reduction='none'),
          floor=case['logits'].double()[:, co:co + nc].abs().max(1).values)


@pytest.mark.parametrize('name,p', DET, ids=lambda v: v if isinstance(v, str) else '')
def test_det_f32_evaluation_lies_inside_the_bound(name, p):
    case, sel = L.det_build(p)
    ref, bound = L.det_loss_statement(**_det_args(case, sel))
    got = L.det_loss_f32(**_det_args(case, sel))
    inside(got['out3'][:2], ref['out3'][:2], bound['out3'][:2], 'losses')
    assert round(float(got['out3'][2]) * ref['rows'] / 100.0) == ref['count']
    inside(got['out3'][2:], ref['out3'][2:], bound['out3'][2:], 'acc')
    inside(got['dlogits'], ref['dlogits'], bound['dlogits'], 'dlogits')
    ce, bce = L.ce_rows_statement(case['logits'], case['cls_off'], case['ncls'], case['labels'])
    inside(F.cross_entropy(case['logits'][:, case['cls_off']:case['cls_off'] + case['ncls']], case['labels'], reduction='none'), ce, bce, 'ce rows')


def test_det_cases_reach_every_branch():
    """What the case builder promises: deltas exactly on +-beta and one ulp-scale step to either side, background rows with box
    weights, rows with zero label weight, a row of logits at +-1e4, and the special kinds."""
    for beta in (1.0, 1.0 / 9.0):
        case, _ = L.det_build(dict(R=4500, layout=L.DET_LAYOUTS[0], beta=beta, kind='plain', sel=None))
        b = L.f32v(beta)
        d = (case['logits'][:, 31:35].double() - case['bbox_t'].double())[case['labels'] > 0]
        for v in (b, -b):
            assert bool((d == v).any())
        assert bool(((d.abs() > b) & (d.abs() < b * (1 + 2.0 ** -19))).any()) and bool(((d.abs() < b) & (d.abs() > b * (1 - 2.0 ** -19))).any())
        assert bool((d == 0).all(1).any())
        assert bool(((case['labels'] == 0)[:, None] & (case['bbox_w'] > 0)).any()) and bool((case['label_w'] == 0).any())
        assert float(case['logits'][:, :31].abs().max()) >= 1e4
    assert int((L.det_build(dict(R=257, layout=L.DET_LAYOUTS[0], beta=1.0, kind='no_pos', sel=None))[0]['labels'] > 0).sum()) == 0
    assert float(L.det_build(dict(R=257, layout=L.DET_LAYOUTS[0], beta=1.0, kind='zero_w', sel=None))[0]['label_w'].abs().sum()) == 0
    big = L.det_build(dict(R=257, layout=L.DET_LAYOUTS[0], beta=1.0, kind='big', sel=None))[0]['logits'][:, :31]
    assert float(big.max()) == 80.0 or float(big.min()) == -80.0


@pytest.mark.parametrize('R', [257, 4500, 20000])
@pytest.mark.parametrize('mistake', L.MISTAKES_DET + L.MISTAKES_DET_SAMPLED)
def test_det_mistakes_exceed_the_bound_tenfold(mistake, R):
    """avg = R instead of max(#{w > 0}, 1); 0.5 a^2 without / beta; the label > 0 gate dropped; log-sum-exp without subtracting the
    maximum (f32, the +-1e4 row); sampled form: smooth-L1 divided by R, accuracy counted over all rows."""
    sel = 'real' if mistake in L.MISTAKES_DET_SAMPLED else None
    case, sc = L.det_build(dict(R=R, layout=L.DET_LAYOUTS[0], beta=1.0 / 9.0, kind='plain', sel=sel))
    ref, bound = L.det_loss_statement(**_det_args(case, sc))
    bad, _ = L.det_loss_statement(mistake=mistake, **_det_args(case, sc))
    which = {'avg_is_R': 0, 'lse_without_max': 0, 'no_div_beta': 1, 'no_label_gate': 1, 'sampled_bbox_over_R': 1, 'sampled_acc_all_rows': 2}[mistake]
    assert bool(moved_tenfold(bad['out3'][which], ref['out3'][which], bound['out3'][which]))
    if mistake == 'sampled_acc_all_rows':
        assert bad['count'] != ref['count']
    if mistake in ('avg_is_R', 'no_label_gate', 'sampled_bbox_over_R'):       # the gradient moves too, on the elements the mistake touches
        touched = (bad['dlogits'] != ref['dlogits'])
        assert int(touched.sum()) > R // 8
        assert bool(moved_tenfold(bad['dlogits'], ref['dlogits'], bound['dlogits'])[touched].all())


def test_statements_reproduce_the_recorded_reference_losses():
    """g12 (RPN loss, OHEM row losses, OHEM loss on the gathered rows) and g11 (the SELSA head's loss on its own logits) were
    recorded from the reference's modules: the statements meet them at the tolerances of those fixtures' own tests."""
    from hvrnet_amd import synthetic as S
    from oracle import hvr_oracle as O
    from tests.golden import cases as C
    g = gold('g12_targets')
    tc = C.target_case()
    # RPN: the fused layout o [rows, 5A] from the reference's [1, A, H, W] / [1, 4A, H, W] maps
    cls, reg = tc['rpn_cls'], tc['rpn_reg']
    A, H, W = cls.shape[1], cls.shape[2], cls.shape[3]
    o = torch.cat([cls[0].permute(1, 2, 0).reshape(H * W, A), reg[0].permute(1, 2, 0).reshape(H * W, 4 * A)], 1).contiguous()
    counts = (int(g['rpn_num_pos']), int(g['rpn_num_neg']))
    ref, _ = L.rpn_loss_statement(o, A, torch.as_tensor(g['rpn_labels']), torch.as_tensor(g['rpn_label_weights']),
                                  torch.as_tensor(g['rpn_bbox_targets']), torch.as_tensor(g['rpn_bbox_weights']), counts, 1.0 / 9.0)
    close(ref['out2'][0], g['loss_rpn_cls'], 1e-5, 1e-6)
    close(ref['out2'][1], g['loss_rpn_bbox'], 1e-5, 1e-6)
    close(ref['d_o'][:, :A].reshape(H, W, A).permute(2, 0, 1), g['d_rpn_cls'][0], 1e-5, 1e-8)
    dreg = ref['d_o'][:, A:5 * A]
    dref = dreg.reshape(H, W, 4 * A).permute(2, 0, 1)
    close(dref[dref != 0], g['d_rpn_reg_nz'], 1e-5, 1e-8)
    assert abs(float(dreg.abs().sum()) - float(g['d_rpn_reg_abs'])) <= 1e-5 * float(g['d_rpn_reg_abs'])
    # OHEM
    labels, bt = torch.as_tensor(g['rcnn_labels']), torch.as_tensor(g['rcnn_bbox_targets'])
    n = labels.shape[0]
    logits = torch.cat([tc['cls_score'][:n], tc['bbox_pred'][:n].view(n, 4)], 1).contiguous()
    ce, _ = L.ce_rows_statement(logits, 0, 31, labels)
    close(ce, g['ohem_row_loss'], 1e-5, 1e-6)
    opos, oneg = torch.as_tensor(g['ohem_pos_inds']).long(), torch.as_tensor(g['ohem_neg_inds']).long()
    lw, bw = torch.zeros(n), torch.zeros(n, 4)
    lw[opos] = 1.0
    lw[oneg] = 1.0
    bw[opos] = 1.0
    ref, _ = L.det_loss_statement(logits, 0, 31, 31, labels, lw, bt, bw, 1.0, sel_counts=(opos.numel(), oneg.numel()))
    close(ref['out3'][0], g['ohem_loss_cls'], 1e-5, 1e-6)
    close(ref['out3'][1], g['ohem_loss_bbox'], 1e-5, 1e-6)
    close(ref['out3'][2], g['ohem_acc'], 1e-5, 1e-5)
    close(ref['dlogits'][:, :31], g['ohem_d_cls'], 1e-5, 1e-8)
    close(ref['dlogits'][:, 31:35], g['ohem_d_reg'], 1e-5, 1e-8)
    # g11: the head's own logits from the host restatement of the SELSA head, then the plain form
    g11 = gold('g11_selsa_train')
    labels, lw, bt, bw = C.head_train_case()
    with torch.no_grad():
        cls, reg = O.selsa_head_forward(C.roi_feat_input(), S.synth_state_dict('selsa'), dict(start=32, length=32), 32, 3)
    logits = torch.cat([cls, reg.view(reg.shape[0], 4)], 1).contiguous()
    ref, _ = L.det_loss_statement(logits, 0, cls.shape[1], cls.shape[1], labels, lw, bt, bw, 1.0)
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'acc')):
        close(ref['out3'][i], g11[k], 1e-5, 1e-6)


# ------------------------------------------------------------------------------------------------ rpn loss
RPN = [(s, c, big) for s in L.RPN_SHAPES for c in L.RPN_COUNTS for big in (False, True)]


def _rpn_case(shape, counts, big):
    rows, A, ldo = shape
    return L.rpn_case(rows, A, ldo, counts, seed=rows + A + counts[1] + int(big), big=big)


def _rpn_args(c):
    return dict(o=c['o'], A=c['A'], labels=c['labels'], label_w=c['label_w'], bbox_t=c['bbox_t'], bbox_w=c['bbox_w'], counts=c['counts'],
                beta=c['beta'])


@pytest.mark.parametrize('shape,counts,big', RPN)
def test_rpn_statement_equals_torch_in_f64_and_f32_lies_inside_the_bound(shape, counts, big):
    c = _rpn_case(shape, counts, big)
    ref, bound = L.rpn_loss_statement(**_rpn_args(c))
    rows, A, ldo = shape
    M = rows * A
    beta = L.f32v(c['beta'])
    o = c['o'].double().requires_grad_(True)
    avg = float(max(counts[0], 1) + max(counts[1], 1))
    lc = (F.binary_cross_entropy_with_logits(o[:, :A].reshape(-1), c['labels'].double(), reduction='none') * c['label_w'].double()).sum() / avg
    l1 = F.smooth_l1_loss(o[:, A:5 * A].reshape(M, 4) / beta, c['bbox_t'].double() / beta, reduction='none') * beta
    lb = (l1 * c['bbox_w'].double()).sum() / avg
    (lc + lb).backward()
    rel12(ref['out2'][0], lc.detach(), floor=1.0)      # torch forms log(1 + exp(-|x|)) without log1p: 2^-53 of 1 per term
    rel12(ref['out2'][1], lb.detach())
    assert torch.allclose(ref['d_o'], o.grad, rtol=1e-12, atol=1e-300 + 1e-15 * float(o.grad.abs().max()))
    assert bool((ref['d_o'][:, 5 * A:] == 0).all())
    got = L.rpn_loss_f32(**_rpn_args(c))
    inside(got['out2'], ref['out2'], bound['out2'], 'losses')
    inside(got['d_o'], ref['d_o'], bound['d_o'], 'd_o')
    if big:
        x = c['o'][:, :A]
        assert float(x.abs().max()) == 90.0 and (M < 100 or (float(x.max()) > 30 and float(x.min()) < -30))
    if M >= 2:
        assert bool((c['o'][:, :A] == 0).any())


@pytest.mark.parametrize('mistake', L.MISTAKES_RPN)
@pytest.mark.parametrize('shape', [(2394, 12, 64), (7, 3, 15)])
def test_rpn_mistakes_exceed_the_bound_tenfold(shape, mistake):
    """c0 + c1 without the max(., 1) (counts with a zero); 0.5 a^2 without / beta; the x < 0 sigmoid taken from the x >= 0 formula."""
    c = _rpn_case(shape, (0, 256), mistake == 'sigmoid_one_branch')
    ref, bound = L.rpn_loss_statement(**_rpn_args(c))
    bad, _ = L.rpn_loss_statement(mistake=mistake, **_rpn_args(c))
    if mistake == 'sigmoid_one_branch':
        A = c['A']
        touched = ((c['o'][:, :A] < 0) & (c['label_w'].view(-1, A) > 0))
        assert int(touched.sum()) > 0
        assert bool(moved_tenfold(bad['d_o'][:, :A], ref['d_o'][:, :A], bound['d_o'][:, :A])[touched].all())
    else:
        which = 0 if mistake == 'avg_without_max' else 1
        assert bool(moved_tenfold(bad['out2'][which], ref['out2'][which], bound['out2'][which]))
        assert bool(moved_tenfold(bad['out2'], ref['out2'], bound['out2']).any())


# ------------------------------------------------------------------------------------------------ sgd
def _torch_sgd(p, g, buf, lr, mom, wd, gscale, max_norm, first, steps=1):
    """torch.optim.SGD + clip_grad_norm_ in f64 on the f32-valued hyper-parameters."""
    P = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.SGD([P], lr=L.f32v(lr), momentum=L.f32v(mom), weight_decay=L.f32v(wd))
    if not first:
        opt.state[P]['momentum_buffer'] = buf.double().clone()
    for _ in range(steps):
        P.grad = g.double() * L.f32v(gscale)
        if max_norm > 0:
            # clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) with the kernel's f32 value of 1e-6
            norm = float(torch.linalg.vector_norm(P.grad))
            P.grad.mul_(min(1.0, L.f32v(max_norm) / (norm + L.f32v(1e-6))))
        opt.step()
    return P.detach(), opt.state[P]['momentum_buffer']


@pytest.mark.parametrize('gscale', [1.0, 0.125])
@pytest.mark.parametrize('n', L.SGD_SIZES)
def test_sgd_statement_equals_torch_and_f32_lies_inside_the_bound(n, gscale):
    p, g, buf = L.sgd_case(n, seed=n)
    for name, max_norm, first, stale in L.sgd_configs(g, gscale):
        b0 = L.sgd_case(n, seed=n, stale=True)[2] if stale else buf
        (rp, rb), (bp, bb), clip = L.sgd_statement(p, g, b0, gscale=gscale, max_norm=max_norm, first=first, **L.SGD_HYPER)
        tp, tb = _torch_sgd(p, g, b0, L.SGD_HYPER['lr'], L.SGD_HYPER['mom'], L.SGD_HYPER['wd'], gscale, max_norm, first)
        floor = g.double().abs() + p.double().abs() + b0.double().abs()       # d = g k + wd p (+ mom buf) may cancel: relative to the operands
        assert bool(((rp - tp).abs() <= 1e-12 * floor).all()) and bool(((rb - tb).abs() <= 1e-12 * floor).all()), name
        fp, fb = L.sgd_f32(p, g, b0, gscale=gscale, max_norm=max_norm, first=first, **L.SGD_HYPER)
        inside(fp, rp, bp, name + ' p')
        inside(fb, rb, bb, name + ' buf')
        if name == 'far_below':
            assert clip < 2e-3
        if name in ('noclip', 'far_above'):
            assert clip == 1.0
        if name in ('ulp_below', 'at_norm', 'ulp_above'):
            assert abs(clip - 1.0) < 4 * L.U
    # torch.clip_grad_norm_ itself agrees with the restated coefficient
    P = torch.nn.Parameter(p.double().clone())
    P.grad = g.double() * L.f32v(gscale)
    torch.nn.utils.clip_grad_norm_([P], 0.01)
    nrm = float(torch.linalg.vector_norm(g.double() * L.f32v(gscale)))
    assert torch.allclose(P.grad, g.double() * L.f32v(gscale) * min(1.0, 0.01 / (nrm + 1e-6)), rtol=1e-12, atol=0)


@pytest.mark.parametrize('mistake', L.MISTAKES_SGD)
def test_sgd_mistakes_exceed_the_bound_tenfold(mistake):
    """The clip norm taken over the un-averaged gradient (grad_scale 1/8); weight decay added after the momentum update; a stale
    buffer used on first_step; the n & 3 tail of the sum of squares dropped (n = 5, 3: the tail is most of the norm)."""
    for n in ((3, 5) if mistake == 'tail_dropped' else (5, 1000003)):
        p, g, buf = L.sgd_case(n, seed=n, stale=(mistake == 'stale_first'))
        lo, mid, hi = L.norm_f32_neighbours(g, 0.125)
        kw = dict(gscale=0.125, max_norm=1e-1 * mid, first=(mistake == 'stale_first'), **L.SGD_HYPER)
        (rp, rb), (bp, bb), _ = L.sgd_statement(p, g, buf, **kw)
        (wp, wb), _, _ = L.sgd_statement(p, g, buf, mistake=mistake, **kw)
        # after ONE step a mistake shows where its term is not negligible: on nine elements in ten at least (a gradient or parameter
        # element near zero has nothing to move); weight decay after the momentum update leaves the first parameter step unchanged
        # (lr wd p is subtracted either way) and shows in the momentum buffer alone -- why the GPU test compares the buffer
        share_p, share_b = float(moved_tenfold(wp, rp, bp).double().mean()), float(moved_tenfold(wb, rb, bb).double().mean())
        assert share_b >= (0.9 if n > 5 else 0.6), (n, 'momentum buffer', share_b)
        if mistake != 'wd_after_momentum':
            assert share_p >= (0.9 if n > 5 else 0.6), (n, 'parameter', share_p)


def test_hvr_flat_buffer_size_takes_the_grid_stride_path():
    """The HVR detector's flat buffer has more float4 chunks than the 1 024 x 256 lanes of the sum of squares: every lane loops."""
    n = L.hvr_flat_numel()
    assert n % 64 == 0 and n // 4 > 1024 * 256
    assert L.sumsq_chain(n) == 4 * -(-(n // 4) // (1024 * 256)) + 21


# ------------------------------------------------------------------------------------------------ relation probs / dscore
CPU_REL = [c for c in L.relation_cases() if c[0] * c[1] <= 300 * 8320]


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('Mq,Mk,D,pad', CPU_REL + [(64, 4500, 1024, 0)])
def test_relation_probs_f32_evaluation_lies_inside_the_bracket(Mq, Mk, D, pad, dtype):
    """softmax(scale q k^T) by torch in f32 (rounded once to the storage type) against the f64 statement: inside the bracket;
    rows sum to one within the summed bound; padding exactly zero.  (The 4 500 x 4 500 window of the GPU tests draws its rows the
    same way; 64 of its rows stand in for it here.)"""
    q, k = L.relation_inputs(Mq, Mk, D, dtype, seed=Mq + Mk, pad=pad)
    sc = L.relation_scale(D)
    P, bound, nt = L.relation_probs_statement(q, k, sc)
    ldp = nt * 128
    got = torch.zeros((Mq, ldp), dtype=dtype)
    got[:, :Mk] = torch.softmax(torch.tensor(sc, dtype=torch.float32) * (q.float() @ k.float().t()), 1).to(dtype)
    lo, hi = L.relation_probs_bracket(P, bound, dtype)
    g = got.double()
    assert bool(((g >= lo) & (g <= hi)).all()), float(((g - P).abs() / bound.clamp(min=1e-300))[(g < lo) | (g > hi)].max())
    assert bool((lo[:, Mk:] == 0).all() and (hi[:, Mk:] == 0).all())
    assert bool(((g.sum(1) - 1).abs() <= (hi - lo).sum(1)).all())
    assert float(bound.max()) < 0.01                      # the bound is a bound, not a blanket
    if Mk >= 2 and D == 1024:                             # the peaky row: its maximum stands more than exp2's f32 range above the other blocks
        assert float(P[0, Mk - 1]) > 1 - 1e-9
        if nt > 1:
            S = sc * (q.double() @ k.double().t())
            assert float(S[0, Mk - 1] - S[0, :128].max()) / math.log(2) > 300


@pytest.mark.parametrize('Mq,Mk', [(37, 4500), (300, 8320), (37, 129)])
def test_relation_neighbour_block_maximum_exceeds_the_bound_tenfold(Mq, Mk):
    """One 128-key block normalised with its neighbour's maximum: every row has elements moved by ten bounds or more, the peaky
    rows by many orders."""
    q, k = L.relation_inputs(Mq, Mk, 1024, torch.float32, seed=Mq + Mk)
    P, bound, nt = L.relation_probs_statement(q, k, 1 / 32)
    bad, _, _ = L.relation_probs_statement(q, k, 1 / 32, mistake='neighbour_max')
    moved = moved_tenfold(bad, P, bound)
    assert bool(moved.any(1)[1:].all())                   # (row 0 is one-hot to f64 precision: a factor on its block changes nothing)
    assert int(moved.sum()) > Mq * Mk // 4


@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
@pytest.mark.parametrize('cancel', [False, True])
@pytest.mark.parametrize('Mq,Mk,D', [(37, 129, 1024), (300, 4500, 1024), (8, 16384, 64), (1, 1, 1024)])
def test_relation_dscore_f32_inside_the_bracket_and_delta_omitted_exceeds_it(Mq, Mk, D, cancel, dtype):
    P, dP, dO, O = L.dscore_inputs(Mq, Mk, D, dtype, seed=Mq + Mk + int(cancel), cancel=cancel)
    sc = L.relation_scale(D)
    ref, bound = L.relation_dscore_statement(P, dP, dO, O, sc)
    delta = (dO.float() * O.float()).sum(1, keepdim=True)
    got = (torch.tensor(sc, dtype=torch.float32) * P.float() * (dP.float() - delta)).to(dtype).double()
    lo, hi = L.bracket(ref, bound, dtype)
    assert bool(((got >= lo) & (got <= hi)).all())
    assert bool((ref[:, Mk:] == 0).all())
    if dtype == torch.float32:
        bad, _ = L.relation_dscore_statement(P, dP, dO, O, sc, mistake='no_delta')
        live = P[:, :Mk].double() > 1e-30
        assert bool(moved_tenfold(bad, ref, bound)[:, :Mk][live].all())
    if cancel:
        d64 = (dO.double() * O.double()).sum(1, keepdim=True)
        assert float(((dP.double() - d64).abs() / d64.abs().clamp(min=1e-3))[:, :Mk].median()) < 2.0 ** -6


# ------------------------------------------------------------------------------------------------ relu_bwd / scale_rows
@pytest.mark.parametrize('dtype', L.RELATION_DTYPES, ids=['f32', 'bf16', 'half'])
def test_relu_case_and_statement(dtype):
    dy, y = L.relu_case(1020, dtype, 3)
    want = L.relu_bwd_statement(dy, y)
    assert not bool(torch.isnan(want[y <= 0]).any()) and bool((want[y <= 0] == 0).all())
    assert float(want[2]) == float(dy[2]) and float(y[2]) > 0           # the smallest subnormal is positive: the gradient passes
    assert bool(torch.isnan(dy[:2]).all()) and float(want[0]) == 0 and float(want[1]) == 0
    assert bool(torch.equal(want[y > 0], dy[y > 0]))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'half'])
@pytest.mark.parametrize('R,C', [(64, 576), (2048, 512), (1, 4)])
def test_scale_rows_ties_separate_one_rounding_from_two(R, C, dtype):
    """The case holds f32 products that are exact ties of the storage type in bulk (s = 1.5, 0.75) and, in the randomly scaled rows,
    searched ones whose f32 value is a tie while the exact product is not: only there may rounding the exact product once (what a
    mixed-precision fma does) differ from the statement, and on about half of them it does."""
    w, s, tie, inexact = L.scale_rows_case(R, C, dtype, seed=R + C)
    two, one = L.scale_rows_statement(w, s), L.scale_rows_single_rounding(w, s)
    differ = two.float() != one.float()
    assert bool((differ <= (tie & inexact)).all())
    if R > 1:
        assert int((tie & ~inexact).sum()) > R * C // 16
        if dtype == torch.float16 or R >= 2048:          # (bf16 ties of inexact products are 2^-16 of all values: the small case may hold none)
            assert int(differ.sum()) >= (R // 16 if dtype == torch.float16 else 1), (int(differ.sum()), int((tie & inexact).sum()))
