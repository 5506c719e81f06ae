"""Generates tests/golden/gcb_modules.json and tests/golden/g23_gcb_block.npz by running the REFERENCE's own context block
(build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_gcb_golden.py

mmdet/ops/context_block.py is loaded where it lies on top of make_golden.py's stub loader, and the real class is assigned over the
dummy `ContextBlock` the loader left in the loaded resnet module (resnext's Bottleneck builds its context block through resnet's).
gcb_modules.json holds, per constructor call, the keywords and the state-dict keys with their shapes in order, in the run-length form
of resnext_modules.json (make_resnext_golden.keys_of).  g23_gcb_block.npz holds, in float64 (randomised weights and BatchNorm
statistics, eval mode; the LAST conv of every branch randomised too -- the reference zeroes it, which makes a fresh block the identity):
  ca.*  ContextBlock(128, 1/8, 'att', ('channel_add', 'channel_mul')) on ca.x [2,128,5,7];
  cb.*  ContextBlock(64, 0.31, 'avg', ('channel_mul',)) on cb.x [2,64,5,3]           (int(64 * 0.31) = int(19.84) = 19: truncated);
  pa.*  a projection Bottleneck(64, 32, stride=2) with gcb (ratio 1/4, att, add + mul) on pa.x [2,64,9,11] (odd sides);
  pb.*  an identity Bottleneck(128, 32) with gcb (ratio 1/16, att, add) on pb.x [1,128,5,7].
Parameters and inputs are drawn in float32 and widened (every stored value is a float32 value); `*.out` is the float64 evaluation,
`*.out_f32` the reference's own float32 evaluation of the same module.  Nothing of the reference is copied: the script executes it
and stores names and numbers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden import make_resnext_golden as RXG  # noqa: E402
from tests.golden import make_res2net_golden as R2G  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

GCB = dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))
SWG = (False, True, True, True)
RESNETS = [dict(depth=depth, gcb=GCB, stage_with_gcb=SWG) for depth in (50, 101)]
RESNEXTS = [dict(depth=101, groups=32, base_width=4, gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', )), stage_with_gcb=SWG)]


def load_reference():
    rx, _ = RXG.load_reference()
    cbm = MG._load('mmdet.ops.context_block', 'mmdet/ops/context_block.py')
    rn = sys.modules['mmdet.models.backbones.resnet']
    rn.ContextBlock = sys.modules['mmdet.ops'].ContextBlock = cbm.ContextBlock
    return rn, rx, cbm


def listed(kw):
    return {k: (listed(v) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}


def randomise32(module, g):
    """make_res2net_golden.randomise32, plus the LayerNorm affines and every conv bias of the context blocks."""
    R2G.randomise32(module, g)
    for m in module.modules():
        if isinstance(m, nn.LayerNorm):
            m.weight.data = (torch.rand(m.weight.shape, generator=g) + 0.5).double()
            m.bias.data = (torch.randn(m.bias.shape, generator=g) * 0.2).double()
        elif isinstance(m, nn.Conv2d) and m.bias is not None:
            m.bias.data = (torch.randn(m.bias.shape, generator=g) * 0.1).double()


def evaluate(arrays, name, module, x, g):
    module = module.double().eval()
    randomise32(module, g)
    with torch.no_grad():
        y = module(x)
        y32 = module.float()(x.float())
    module.double()
    assert y.dtype == torch.float64 and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
    for k, v in module.state_dict().items():
        arrays['%s.%s' % (name, k)] = v
    arrays['%s.x' % name], arrays['%s.out' % name], arrays['%s.out_f32' % name] = x, y, y32
    print('%s: out %s, |out| max %.3f, f32 run off by %.2e' % (name, tuple(y.shape), float(y.abs().max()), float((y32.double() - y).abs().max())))


def main():
    rn, rx, cbm = load_reference()
    cases = []
    for cls, mod, kws in (('ResNet', rn, RESNETS), ('ResNeXt', rx, RESNEXTS)):
        for kw in kws:
            net = getattr(mod, cls)(**kw)
            cases.append(dict(cls=cls, kwargs=listed(kw), runs=RXG.keys_of(net)))
            print('%s %s: %d runs, %d keys' % (cls, kw, len(cases[-1]['runs']), len(net.state_dict())))
    path = os.path.join(MG.OUT, 'gcb_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/ops/context_block.py', 'mmdet/models/backbones/resnet.py', 'mmdet/models/backbones/resnext.py'],
                       suffixes=RXG.SUFFIXES, templates=RXG.TEMPLATES, cases=cases), f, sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    g = torch.Generator().manual_seed(23)
    arrays = {}
    evaluate(arrays, 'ca', cbm.ContextBlock(128, 1. / 8., 'att', ('channel_add', 'channel_mul')), torch.randn((2, 128, 5, 7), generator=g).double(), g)
    evaluate(arrays, 'cb', cbm.ContextBlock(64, 0.31, 'avg', ('channel_mul', )), torch.randn((2, 64, 5, 3), generator=g).double(), g)
    down = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    evaluate(arrays, 'pa', rn.Bottleneck(64, 32, stride=2, downsample=down, gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))),
             torch.randn((2, 64, 9, 11), generator=g).double(), g)
    evaluate(arrays, 'pb', rn.Bottleneck(128, 32, gcb=dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', ))),
             torch.randn((1, 128, 5, 7), generator=g).double(), g)
    MG.save('g23_gcb_block', **arrays)


if __name__ == '__main__':
    main()
