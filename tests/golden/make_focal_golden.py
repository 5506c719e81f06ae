"""Generates tests/golden/focal.npz by running the REFERENCE's own focal-loss and sampling-free anchor-target code (build container
only; needs the reference tree at make_golden.REF):

    python tests/golden/make_focal_golden.py

mmdet/models/losses/focal_loss.py is loaded where it lies on top of make_golden.py's stub loader.  It imports the compiled op
`mmdet.ops.sigmoid_focal_loss`, which cannot run here and is stubbed with None: what runs is the file's `py_sigmoid_focal_loss` (the
formula BCEWithLogits x (alpha t + (1 - alpha)(1 - t)) pt^gamma) with losses/utils.py `weight_reduce_loss`, in float64, and torch's
autograd for the gradient.  Per case <k> (logits, int targets 0 = background / c + 1 = class c, row weights, gamma, alpha):
  <k>.none                                     reduction 'none', no weight          [N, C]
  <k>.mean / .mean_avg / .sum                  with the row weights; .mean_avg with avg_factor = <k>.avg
  <k>.grad_sum                                 d <k>.sum / d logits                 [N, C]
and the reference's anchor_target(..., sampling=False) (anchor_target.py:7-155 with its PseudoSampler) on a 4 x 5 grid of 3 anchors per
position with 2 ground-truth boxes: at.labels / label_weights / bbox_targets / bbox_weights / num_pos / num_neg beside its inputs.
Nothing of the reference is copied: the script executes it and stores numbers.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.focal_refs import AT_CFG  # noqa: E402  (the train_cfg.rpn of the anchor-target case: stated once, beside the host restatement)

# case: (N, C, gamma, alpha, logit scale, seed)
CASES = dict(a=(9, 4, 2.0, 0.25, 4.0, 271), b=(6, 1, 0.0, 0.5, 4.0, 272), c=(5, 3, 1.5, 0.75, 3.0, 273))
AT_GRID, AT_STRIDE, AT_SCALES, AT_IMG = (4, 5), 16, [1.5, 2.5, 4.0], (60, 76, 3)
AT_GT = [[10.0, 8.0, 49.0, 47.0], [40.0, 20.0, 70.0, 55.0]]


def main():
    ref = MG.install_reference()
    sys.modules['mmdet.ops'].sigmoid_focal_loss = None      # the compiled op: never called here
    fl = MG._load('mmdet.models.losses.focal_loss', 'mmdet/models/losses/focal_loss.py')
    arrays = {}
    for name, (N, C, gamma, alpha, scale, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn((N, C), generator=g) * scale).double().requires_grad_(True)
        t = torch.randint(0, C + 1, (N,), generator=g)
        t[0], t[N - 1] = 0, C
        w = (0.5 + torch.rand(N, generator=g)).double()
        w[1] = 0.0
        onehot = (t[:, None] == torch.arange(1, C + 1)[None, :]).double()
        avg = 7.0
        none = fl.py_sigmoid_focal_loss(x, onehot, None, gamma, alpha, 'none')
        mean = fl.py_sigmoid_focal_loss(x, onehot, w.view(-1, 1), gamma, alpha, 'mean')
        mean_avg = fl.py_sigmoid_focal_loss(x, onehot, w.view(-1, 1), gamma, alpha, 'mean', avg)
        total = fl.py_sigmoid_focal_loss(x, onehot, w.view(-1, 1), gamma, alpha, 'sum')
        grad, = torch.autograd.grad(total, x)
        arrays.update({name + '.x': x.detach(), name + '.t': t, name + '.w': w, name + '.gamma_alpha': np.array([gamma, alpha]),
                       name + '.avg': np.array(avg), name + '.none': none.detach(), name + '.mean': mean.detach(),
                       name + '.mean_avg': mean_avg.detach(), name + '.sum': total.detach(), name + '.grad_sum': grad})
        print('%s: N=%d C=%d sum=%.6g' % (name, N, C, float(total)))

    anchors = ref.AnchorGenerator(AT_STRIDE, AT_SCALES, [1.0]).grid_anchors(AT_GRID, AT_STRIDE, device='cpu')
    valid = torch.ones(anchors.shape[0], dtype=torch.uint8)
    gts = torch.tensor(AT_GT)
    meta = dict(img_shape=AT_IMG, pad_shape=(64, 80, 3), scale_factor=1.0, flip=False)
    lab, lw, bt, bw, npos, nneg = ref.anchor_target([[anchors]], [[valid]], [gts], [meta], [0., 0., 0., 0.], [1., 1., 1., 1.],
                                                    MG.AttrDict(AT_CFG), sampling=False)
    arrays.update({'at.anchors': anchors, 'at.gt_bboxes': gts, 'at.img_shape': np.array(AT_IMG), 'at.labels': lab[0],
                   'at.label_weights': lw[0], 'at.bbox_targets': bt[0], 'at.bbox_weights': bw[0], 'at.num_pos': np.array(npos),
                   'at.num_neg': np.array(nneg)})
    n = anchors.shape[0]
    print('anchor_target(sampling=False): %d anchors, %d pos, %d neg, %d with weight 0' % (n, npos, nneg, int((lw[0] == 0).sum())))
    MG.save('focal', **arrays)


if __name__ == '__main__':
    main()
