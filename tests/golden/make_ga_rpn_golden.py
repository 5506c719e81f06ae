"""Generates tests/golden/g26_ga_rpn.npz and tests/golden/ga_rpn_modules.json by running the REFERENCE's own Guided Anchoring RPN code
(build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_ga_rpn_golden.py

mmdet/models/anchor_heads/guided_anchor_head.py and ga_rpn_head.py are loaded where they lie on top of make_golden.py's stub loader;
`mmdet.ops.nms` is the oracle's NMS (the reference's nms_cpu.cpp, compiled unmodified).  `DeformConv` and `MaskedConv2d` import
compiled CUDA modules and cannot run here: for the KEY LIST they are stubbed inside this script with parameter-only stand-ins (an
nn.Conv2d subclass for MaskedConv2d, which is what the reference's class is; a module with the one `weight` parameter
dcn/deform_conv.py:190-230 registers -- its constructor asserts `not bias` -- for DeformConv), and the losses are not built
(focal_loss.py imports a compiled op too).  So there is NO golden for the forward chain: tests/ga_rpn_refs.py's f64 statement is the
reference there.  What the reference computes here, in its own float32 on the CPU, per case and frame:
  GuidedAnchorHead.get_guided_anchors_single(squares, shape_pred, loc_pred, use_loc_filter=True)  -> <case>.f<t>.anchors, .mask
  GARPNHead.get_bboxes_single([cls], [reg], [anchors], [mask], img_shape, 1.0, cfg)              -> <case>.f<t>.proposals
on prescribed random maps (<case>.cls / reg / shape / loc, [T,H,W,*] float32).  A frame with no kept pixel is not in the fixture: the
reference `continue`s past the level and fails in torch.cat.  ga_rpn_modules.json holds the constructor keywords and the state-dict
keys with their shapes, in order.  Nothing of the reference is copied: the script executes it and stores names and numbers.
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

HEAD_KW = dict(in_channels=64, feat_channels=64, octave_base_scale=2, scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0], anchor_strides=[16],
               anchoring_means=[0.1, -0.05, 0.02, 0.03], anchoring_stds=[0.07, 0.07, 0.14, 0.14], target_means=[0.0, 0.0, 0.0, 0.0],
               target_stds=[0.07, 0.07, 0.11, 0.11], deformable_groups=4, loc_filter_thr=0.01)
FULL_KW = dict(HEAD_KW, in_channels=1024, feat_channels=1024, octave_base_scale=8)
# case: (T, H, W, img_shape, loc_filter_thr, dict(nms_pre, nms_post, max_num, nms_thr), seed)
CASES = dict(
    a=(3, 5, 7, (80, 112), 0.01, dict(nms_pre=12, nms_post=10, max_num=9, nms_thr=0.7), 261),
    b=(2, 9, 11, (140, 170), 0.3, dict(nms_pre=0, nms_post=300, max_num=300, nms_thr=0.5), 262),
    c=(2, 5, 7, (80, 112), 0.5, dict(nms_pre=1000, nms_post=5, max_num=12, nms_thr=0.7), 263),     # thr 0.5 with logits exactly 0: sigmoid == thr
)


def load_reference():
    ref = MG.install_reference()
    ops, core = sys.modules['mmdet.ops'], sys.modules['mmdet.core']

    class MaskedConv2d(nn.Conv2d):      # parameter-only stand-in (masked_conv.py:64-89 is an nn.Conv2d subclass too)
        pass

    class DeformConv(nn.Module):        # parameter-only stand-in: dcn/deform_conv.py:190-230 registers `weight` alone (asserts `not bias`)
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
            super(DeformConv, self).__init__()
            assert not bias
            self.weight = nn.Parameter(torch.zeros(out_channels, in_channels // groups, kernel_size, kernel_size))

    ops.MaskedConv2d, ops.DeformConv = MaskedConv2d, DeformConv
    for n in ('anchor_inside_flags', 'ga_loc_target', 'ga_shape_target'):     # training only
        setattr(core, n, None)
    wi = MG._load('mmdet.models.utils.weight_init', 'mmdet/models/utils/weight_init.py')
    sys.modules['mmdet.models.utils'].bias_init_with_prob = wi.bias_init_with_prob
    gah = MG._load('mmdet.models.anchor_heads.guided_anchor_head', 'mmdet/models/anchor_heads/guided_anchor_head.py')
    gah.build_loss = lambda cfg: None   # FocalLoss imports a compiled op; the losses are training only
    gar = MG._load('mmdet.models.anchor_heads.ga_rpn_head', 'mmdet/models/anchor_heads/ga_rpn_head.py')
    return ref, gah, gar


def maps_of(T, H, W, thr, seed):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn((T, H, W, 1), generator=g) * 2.0
    reg = torch.randn((T, H, W, 4), generator=g) * 3.0
    shape = torch.randn((T, H, W, 2), generator=g) * 4.0
    loc = torch.randn((T, H, W, 1), generator=g) * 2.0 + math.log(thr / (1.0 - thr))
    shape[:, 0, 0, 0], shape[:, 1, 2, 1], shape[:, 2, 3, 0] = 120.0, -110.0, 99.0     # x 0.14: beyond the 1e-6 clip (13.8) on both sides
    loc[:, 0, 0], loc[:, 1, 2], loc[:, 2, 3] = 5.0, 5.0, 5.0                          # ... at kept pixels
    if thr == 0.5:
        loc[:, 0, 1:4], loc[:, 3, 3] = 0.0, 0.0                                       # sigmoid(0) == 0.5 == thr in any arithmetic: kept by >=
    if T > 1 and (H, W) == (9, 11):
        loc[1] = -20.0
        loc[1, 4, 6] = 3.0                                                            # a frame with ONE kept pixel
    return cls, reg, shape, loc


def main():
    ref, gah, gar = load_reference()
    cases = []
    for kw in (HEAD_KW, FULL_KW):
        head = gar.GARPNHead(**kw)
        cases.append(dict(cls='GARPNHead', kwargs=kw, keys=[[k, list(v.shape)] for k, v in head.state_dict().items()]))
        print('GARPNHead(%d): %d keys' % (kw['in_channels'], len(cases[-1]['keys'])))
    path = os.path.join(MG.OUT, 'ga_rpn_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/anchor_heads/ga_rpn_head.py', 'mmdet/models/anchor_heads/guided_anchor_head.py',
                               'mmdet/ops/masked_conv/masked_conv.py', 'mmdet/ops/dcn/deform_conv.py'],
                       stubbed=['mmdet.ops.DeformConv', 'mmdet.ops.MaskedConv2d', 'mmdet.models.builder.build_loss'], cases=cases), f,
                  sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    arrays = {}
    for name, (T, H, W, img_shape, thr, cfg, seed) in CASES.items():
        head = gar.GARPNHead(**dict(HEAD_KW, loc_filter_thr=thr)).eval()
        cls, reg, shape, loc = maps_of(T, H, W, thr, seed)
        squares = head.square_generators[0].grid_anchors((H, W), head.anchor_strides[0], device='cpu')
        arrays['%s.cls' % name], arrays['%s.reg' % name], arrays['%s.shape' % name], arrays['%s.loc' % name] = cls, reg, shape, loc
        arrays['%s.squares' % name] = squares
        arrays['%s.meta' % name] = np.array([img_shape[0], img_shape[1], thr, cfg['nms_pre'], cfg['nms_post'], cfg['max_num'], cfg['nms_thr']],
                                            dtype=np.float64)
        c = MG.AttrDict(dict(cfg, min_bbox_size=0, nms_across_levels=False))
        for t in range(T):
            anchors, mask = head.get_guided_anchors_single(squares, shape[t].permute(2, 0, 1), loc[t].permute(2, 0, 1), use_loc_filter=True)
            props = head.get_bboxes_single([cls[t].permute(2, 0, 1)], [reg[t].permute(2, 0, 1)], [anchors], [mask], img_shape + (3, ), 1.0, c)
            arrays['%s.f%d.anchors' % (name, t)], arrays['%s.f%d.mask' % (name, t)] = anchors, mask.to(torch.uint8)
            arrays['%s.f%d.proposals' % (name, t)] = props
            print('%s frame %d: %d kept of %d, %d proposals' % (name, t, int(mask.sum()), H * W, props.shape[0]))
    MG.save('g26_ga_rpn', **arrays)


if __name__ == '__main__':
    main()
