"""Generates tests/golden/losses.npz by running the REFERENCE's own loss functions and classes (build container only; needs the
reference tree at make_golden.REF):

    python tests/golden/make_losses_golden.py

mmdet/models/losses/{smooth_l1_loss, balanced_l1_loss, mse_loss, iou_loss, ghm_loss}.py are loaded where they lie on top of
make_golden.py's stub loader and run on the CPU in float64, with torch's autograd for the gradients.  The inputs come from the case
generators of tests/loss_refs.py (f32 values, away from the kinks of the rules; the GHM inputs keep every valid element's g 1e-5 away
from a bin edge).  Per rule <r> in smooth_l1 / balanced_l1 / mse / iou / bounded_iou and case <k> in a / b:
  <r>.<k>.pred / .target / .w / .prm (the rule's parameters, in the order PRM[<r>]) / .avg
  <r>.<k>.none                       reduction 'none', no weight
  <r>.<k>.mean                       reduction 'mean', no weight
  <r>.<k>.mean_w / .mean_avg / .sum_w    with the weights; .mean_avg with avg_factor = .avg
  <r>.<k>.grad_sum_w                 d <k>.sum_w / d pred
  (mse: only .mean of these -- the reference's mse_loss averages before it weights, see the note in main)
  <r>.<k>.tie                        rows on which a max / min of the rule ties (identical boxes): autograd splits the gradient there
and per GHM run <g> in ghmc_m0 (int64 labels through _expand_binary_labels, momentum 0), ghmc_m75, ghmr_m0, ghmr_m75 and call <i> in
0 .. 2 (three consecutive calls on ONE module): <g>.<i>.pred / .target / .weight (as handed to the module), .loss, .grad (d loss /
d pred), .acc_sum (the buffer after the call, momentum 0.75 only); <g>.edges, <g>.cfg = (bins, momentum, loss_weight, mu).
Nothing of the reference is copied: the script executes it and stores numbers.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import loss_refs as R  # noqa: E402

from tests.loss_refs import AVG, CASES, GHM_MU, GHM_RUNS, GHM_SHAPE, PRM  # noqa: E402  (stated once, beside the statements: the tests must not import this maker)


def main():
    MG.install_reference()
    sys.modules['mmdet.core'].bbox_overlaps = sys.modules['mmdet.core.bbox.geometry'].bbox_overlaps      # the stub package lacks the re-export
    mods = {n: MG._load('mmdet.models.losses.' + n, 'mmdet/models/losses/%s.py' % n) for n in ('balanced_l1_loss', 'mse_loss', 'iou_loss', 'ghm_loss')}
    sl1 = sys.modules['mmdet.models.losses.smooth_l1_loss']
    fns = dict(smooth_l1=sl1.smooth_l1_loss, balanced_l1=mods['balanced_l1_loss'].balanced_l1_loss, mse=mods['mse_loss'].mse_loss,
               iou=mods['iou_loss'].iou_loss, bounded_iou=mods['iou_loss'].bounded_iou_loss)
    arrays = {}
    for rule, cases in CASES.items():
        for k, (shape, prm) in cases.items():
            seed = 400 + len(arrays)
            if rule in ('iou', 'bounded_iou'):
                pred, target, w_row, w_elem = R.box_case(shape, seed, beta=prm.get('beta', 0.2), eps=prm['eps'], iou_eps=prm['eps'])
                w = w_row if rule == 'iou' else w_elem
                # rows on which a max / min of the rule compares two equal operands (autograd splits the gradient there; the header names a side)
                if rule == 'iou':
                    tie = (pred == target).any(1)
                else:
                    size, ctr = pred[:, 2:] - pred[:, :2], pred[:, 2:] + pred[:, :2]
                    tie = ((size == target[:, 2:] - target[:, :2]) | (ctr == target[:, 2:] + target[:, :2])).any(1)
            else:
                pred, target, w = R.reg_case(shape[0], shape[1], seed, beta=prm.get('beta', 1.0))
                tie = torch.zeros(shape[0], dtype=torch.bool)
            x = pred.double().requires_grad_(True)
            t, wd = target.double(), w.double()
            fn = fns[rule]
            none = fn(x, t, reduction='none', **prm)
            mean = fn(x, t, reduction='mean', **prm)
            mean_w = fn(x, t, wd, reduction='mean', **prm)
            mean_avg = fn(x, t, wd, reduction='mean', avg_factor=AVG, **prm)
            sum_w = fn(x, t, wd, reduction='sum', **prm)
            grad, = torch.autograd.grad(sum_w, x)
            p = '%s.%s.' % (rule, k)
            arrays.update({p + 'pred': pred, p + 'target': target, p + 'w': w, p + 'prm': np.array([prm[n] for n in PRM[rule]], dtype=np.float64),
                           p + 'avg': np.array(AVG), p + 'none': none.detach(), p + 'mean': mean.detach(), p + 'mean_w': mean_w.detach(),
                           p + 'mean_avg': mean_avg.detach(), p + 'sum_w': sum_w.detach(), p + 'grad_sum_w': grad, p + 'tie': tie})
            if rule == 'mse':      # mse_loss.py:7 wraps F.mse_loss, which averages BEFORE weight_reduce_loss sees the elements: only the unweighted
                for key in ('none', 'mean_w', 'mean_avg', 'sum_w', 'grad_sum_w'):      # 'mean' is the rule's mean of d d; the rest is not stored
                    del arrays[p + key]
            print('%s%s sum_w=%.6g' % (p, tuple(pred.shape), float(sum_w.detach())))

    ghm = mods['ghm_loss']
    # GHMC casts its target with .float(); F.binary_cross_entropy_with_logits would then sum in f32.  The module's namespace gets an F whose
    # binary_cross_entropy_with_logits promotes target and weight to the logits' dtype first, so the run stays in f64 (the file is untouched).
    import types
    import torch.nn.functional as F

    def bce_f64(input, target, weight=None, **kw):
        return F.binary_cross_entropy_with_logits(input, target.to(input.dtype), None if weight is None else weight.to(input.dtype), **kw)
    ghm.F = types.SimpleNamespace(binary_cross_entropy_with_logits=bce_f64)
    for name, (kind, bins, momentum, loss_weight, by_label) in GHM_RUNS.items():
        module = (ghm.GHMC(bins=bins, momentum=momentum, loss_weight=loss_weight) if kind == 'ghmc'
                  else ghm.GHMR(mu=GHM_MU, bins=bins, momentum=momentum, loss_weight=loss_weight)).double()
        arrays[name + '.edges'] = module.edges.float()
        arrays[name + '.cfg'] = np.array([bins, momentum, loss_weight, GHM_MU])
        for i in range(3):
            c = R.ghm_case(kind, GHM_SHAPE[0], GHM_SHAPE[1], bins, seed=500 + 10 * len(name) + i, mu=GHM_MU, labels=by_label)
            assert bool((c['edges'] == module.edges.float()).all())
            x = c['pred'].double().requires_grad_(True)
            if by_label:
                target, weight = c['labels'], c['label_weight']
                loss = module(x, target, weight.double())
            else:
                target, weight = c['target'], c['weight']
                loss = module(x, target.double(), weight.double())
            grad, = torch.autograd.grad(loss, x)
            p = '%s.%d.' % (name, i)
            arrays.update({p + 'pred': c['pred'], p + 'target': target, p + 'weight': weight, p + 'loss': loss.detach(), p + 'grad': grad})
            if momentum > 0:
                arrays[p + 'acc_sum'] = module.acc_sum.detach().clone()
            print('%sloss=%.6g' % (p, float(loss)))
    MG.save('losses', **arrays)


if __name__ == '__main__':
    main()
