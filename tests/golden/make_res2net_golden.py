"""Generates tests/golden/res2net_modules.json and tests/golden/g22_res2net_block.npz by running the REFERENCE's own Res2Net code
(build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_res2net_golden.py

mmdet/models/backbones/res2net_v1b.py and mmdet/models/shared_heads/res2_layer.py are loaded where they lie on top of make_golden.py's
stub loader, as make_resnext_golden.py loads the ResNeXt files.  res2net_modules.json holds, per constructor call, the keywords and the
state-dict keys with their shapes in order, in the run-length form of resnext_modules.json (make_resnext_golden.keys_of).
g22_res2net_block.npz holds, in float64 (randomised weights and BatchNorm statistics, eval mode):
  a.*     Bottle2neck(64, 32, stride=2, stype='stage') with make_res2_layer's pool -> 1x1 -> BN shortcut, on a.x [2,64,9,11]
          (both sides odd: the ceil-mode shortcut pool has edge windows of 2 and 1 elements);
  b.*     Bottle2neck(128, 32, stype='normal', dilation=2) on b.x [1,128,7,9];
  stem.*  Res2Net's conv1 (three 3x3 convs) + bn1 + ReLU + max pool on stem.x [1,3,33,41];
planes = 32 gives width = 13, so that the padding of a slice to 32 channels is exercised and the file stays small.  Parameters and
inputs are drawn in float32 and widened (every stored value is a float32 value: the file compresses, and a float32 run of the same
module reads the same numbers); `*.out` is the float64 evaluation, `*.out_f32` the reference's own float32 evaluation of the same
module.  Res2Layer.forward does not run under the stub auto_fp16; nothing here calls it.  Nothing of the reference is copied: the
script executes it and stores names and numbers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden import make_resnext_golden as RXG  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

BACKBONES = [dict(num_stages=ns, strides=(1, 2, 2, 2)[:ns], dilations=(1, 1, 1, 1)[:ns], out_indices=(ns - 1,)) for ns in (3, 4)]
HEADS = [dict(depth=101, stage=3, stride=1, dilation=2, external_conv=True)]


def load_reference():
    MG.install_reference()
    bb = sys.modules['mmdet.models.backbones']
    r2 = MG._load('mmdet.models.backbones.res2net_v1b', 'mmdet/models/backbones/res2net_v1b.py')
    bb.Res2Net, bb.make_res2_layer = r2.Res2Net, r2.make_res2_layer
    r2l = MG._load('mmdet.models.shared_heads.res2_layer', 'mmdet/models/shared_heads/res2_layer.py')
    return r2, r2l


def randomise32(module, g):
    """make_resnext_golden.randomise with every value a float32 value."""
    RXG.randomise(module, g)
    for t in list(module.parameters()) + list(module.buffers()):
        if t.is_floating_point():
            t.data = t.data.float().double()


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
    r2, r2l = load_reference()
    cases = []
    for kw in BACKBONES:
        cases.append(dict(cls='Res2Net', kwargs=RXG.listed(kw), runs=RXG.keys_of(r2.Res2Net(**kw))))
        print('Res2Net %s: %d runs, %d keys' % (kw, len(cases[-1]['runs']), len(r2.Res2Net(**kw).state_dict())))
    for kw in HEADS:
        cases.append(dict(cls='Res2Layer', kwargs=RXG.listed(kw), runs=RXG.keys_of(r2l.Res2Layer(**kw))))
        print('Res2Layer %s: %d runs' % (kw, len(cases[-1]['runs'])))
    path = os.path.join(MG.OUT, 'res2net_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/backbones/res2net_v1b.py', 'mmdet/models/shared_heads/res2_layer.py'], suffixes=RXG.SUFFIXES,
                       templates=RXG.TEMPLATES, cases=cases), f, sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    g = torch.Generator().manual_seed(22)
    arrays = {}
    layer = r2.make_res2_layer(r2.Bottle2neck, 64, 32, 1, baseWidth=26, scale=4, stride=2)   # one 'stage' block with its shortcut
    assert layer[0].stype == 'stage' and layer[0].width == 13 and layer[0].downsample is not None
    evaluate(arrays, 'a', layer[0], torch.randn((2, 64, 9, 11), generator=g).double(), g)
    evaluate(arrays, 'b', r2.Bottle2neck(128, 32, baseWidth=26, scale=4, stype='normal', dilation=2), torch.randn((1, 128, 7, 9), generator=g).double(), g)
    net = r2.Res2Net(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    stem = nn.Sequential()
    for n in ('conv1', 'bn1', 'relu', 'maxpool'):
        stem.add_module(n, getattr(net, n))
    evaluate(arrays, 'stem', stem, torch.randn((1, 3, 33, 41), generator=g).double() * 50.0, g)
    MG.save('g22_res2net_block', **arrays)


if __name__ == '__main__':
    main()
