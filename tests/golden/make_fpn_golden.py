"""Generates tests/golden/g27_fpn.npz and tests/golden/fpn_modules.json by running the REFERENCE's own FPN and SingleRoIExtractor
(build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_fpn_golden.py

mmdet/models/necks/fpn.py, mmdet/models/utils/conv_module.py and mmdet/models/roi_extractors/single_level.py are executed where they lie
on top of make_golden.py's stub loader.  Nothing of the reference is copied: the script runs it and stores names and numbers.

FPN part.  The configurations of tests/fpn_refs.CONFIGS (Faster R-CNN style; RetinaNet style, on the inputs and on the outputs with ReLU;
end_level=3 with activation='relu'), in_channels [32, 64, 128, 256], out_channels 32, B = 2 on 16x24, 8x12, 4x6 and 2x3 maps.  Weights
are small integers x 2^-8 and inputs integers x 2^-10, exactly representable in f32; the reference module is converted to f64 and
evaluated there (<name>.out<i>).  fpn_modules.json holds, per configuration, the constructor keywords and the state-dict keys with shapes.

Extractor part.  The reference's SingleRoIExtractor with `mmdet.ops.RoIAlign` bound to oracle.hvr_oracle.roi_align -- its RoIAlign has no
CPU path and roi_align_kernel.cu cannot be built here, exactly as for make_g4.py: the pooled numbers come from this build's C
restatement, the level mapping, the rescaling and the gather / scatter loop from the reference (`ext.roi_align_source = "oracle"`).
Four maps of C = 8 of a 96 x 160 image (strides 4 .. 32), 96 RoIs that reach every level with the boundary boxes of finest_scale = 56
among them, no NaN-scale RoI; `ext.out` plain, `ext.out_rescaled` with roi_scale_factor = 1.5 on the first 32 RoIs.  The script asserts
that the comparison rule of include/hvr_hip.h (tests/fpn_refs.level_rule) equals the reference's levels on every stored RoI and stores them.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import hvr_oracle as O  # noqa: E402
from tests import fpn_refs as R  # noqa: E402

MAPS = [(16, 24), (8, 12), (4, 6), (2, 3)]
EXT_MAPS = [(24, 40), (12, 20), (6, 10), (3, 5)]
EXT_STRIDES = [4, 8, 16, 32]


def load_reference():
    MG.install_reference()
    ops = sys.modules['mmdet.ops']

    class RoIAlign(nn.Module):          # the reference's layer signature (roi_align.py:57-87) over the oracle's C restatement
        def __init__(self, out_size, spatial_scale, sample_num=0, use_torchvision=False):
            super(RoIAlign, self).__init__()
            self.out_size = (out_size, out_size) if isinstance(out_size, int) else out_size
            self.spatial_scale, self.sample_num = float(spatial_scale), int(sample_num)

        def forward(self, features, rois):
            return O.roi_align(features, rois, self.out_size, self.spatial_scale, self.sample_num)

    ops.RoIAlign = RoIAlign
    MG._pkg('mmdet.models.necks')
    fpn = MG._load('mmdet.models.necks.fpn', 'mmdet/models/necks/fpn.py')
    MG._pkg('mmdet.models.roi_extractors')
    sl = MG._load('mmdet.models.roi_extractors.single_level', 'mmdet/models/roi_extractors/single_level.py')
    return fpn.FPN, sl.SingleRoIExtractor


def ext_rois(seed=271, n=96, img=(96, 160)):
    g = torch.Generator().manual_seed(seed)
    ih, iw = img
    side = 8.0 * torch.exp(torch.rand((n, 2), generator=g) * np.log(80.0))            # 8 .. 640 px, log-uniform: every level
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([float(iw), float(ih)])
    box = torch.cat([ctr - side / 2, ctr + side / 2], 1)
    rois = torch.cat([torch.randint(0, 2, (n, 1), generator=g).float(), box], 1)
    b = torch.from_numpy(R.boundary_boxes(x0=-20.0, y0=-30.0))
    rois[8:8 + len(b), 1:] = b
    rois[0, 1:] = torch.tensor([0., 0., iw - 1., ih - 1.])
    rois[1, 1:] = torch.tensor([50., 60., 50., 60.])                                 # a single pixel
    rois[2] = torch.tensor([1., -300., -200., 500., 400.])                           # far beyond the image, batch index B - 1
    return rois


def main():
    FPN, Extractor = load_reference()
    arrays, cases = {}, []
    g = torch.Generator().manual_seed(27)
    xs = [torch.randint(-4096, 4097, (2, c, h, w), generator=g).float() / 1024 for c, (h, w) in zip(R.IN_CHANNELS, MAPS)]
    for i, x in enumerate(xs):
        arrays['x%d' % i] = x
    for name, kw in R.CONFIGS.items():
        m = FPN(**kw)
        for k, p in m.state_dict().items():
            p.copy_(torch.randint(-24, 25, p.shape, generator=g).float() / 256)
        cases.append(dict(name=name, cls='FPN', kwargs=kw, keys=[[k, list(v.shape)] for k, v in m.state_dict().items()]))
        for k, v in m.state_dict().items():
            arrays['%s.%s' % (name, k)] = v.clone()
        with torch.no_grad():
            outs = m.double()([x.double() for x in xs])
        for i, o in enumerate(outs):
            arrays['%s.out%d' % (name, i)] = o
        print('%s: %d keys, outs %s' % (name, len(cases[-1]['keys']), [tuple(o.shape) for o in outs]))
    path = os.path.join(MG.OUT, 'fpn_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/necks/fpn.py', 'mmdet/models/utils/conv_module.py'], cases=cases), f, sort_keys=True, indent=None,
                  separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    ext = Extractor(dict(type='RoIAlign', out_size=7, sample_num=2), 8, EXT_STRIDES, finest_scale=56)
    feats = [torch.randn((2, 8, h, w), generator=g) for h, w in EXT_MAPS]
    rois = ext_rois()
    levels = ext.map_roi_levels(rois, 4)
    mine = R.level_rule(rois.numpy(), 56, 4)
    assert np.array_equal(mine, levels.numpy()), np.nonzero(mine != levels.numpy())
    assert set(levels.tolist()) == {0, 1, 2, 3} and not bool(torch.isnan(rois).any())
    assert np.array_equal(R.level_rule(rois[:32].numpy(), 56, 4), ext.map_roi_levels(rois[:32], 4).numpy())
    for i, f in enumerate(feats):
        arrays['ext.feat%d' % i] = f
    arrays['ext.rois'], arrays['ext.levels'] = rois, levels.int()
    arrays['ext.roi_align_source'] = np.array('oracle')
    with torch.no_grad():
        arrays['ext.out'] = ext(feats, rois)
        arrays['ext.out_rescaled'] = ext(feats, rois[:32], roi_scale_factor=1.5)
    print('extractor: levels', np.bincount(levels.numpy(), minlength=4).tolist())
    MG.save('g27_fpn', **arrays)


if __name__ == '__main__':
    main()
