"""Generates tests/golden/gn_modules.json and tests/golden/g25_gn_block.npz by running the REFERENCE's own ResNet code under
norm_cfg = dict(type='GN', num_groups=...) (build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_gn_golden.py

mmdet/models/backbones/resnet.py and mmdet/models/shared_heads/res_layer.py are the modules make_golden.install_reference loads through
its stub loader.  gn_modules.json holds, per constructor call, the keywords and the state-dict keys with their shapes, in order, in the
run-length form of resnext_modules.json (make_resnext_golden.keys_of: runs of consecutive blocks of a stage that share one form, each
naming an entry of shared tables of key suffixes and shapes); g25_gn_block.npz holds two of the reference's resnet.Bottleneck blocks
under GroupNorm in float64 (randomised weights, gamma and beta), their parameters, one input and their outputs.  Nothing of the
reference is copied: the script executes it and stores names and numbers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden import make_resnext_golden as RX  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

GN = dict(type='GN', num_groups=32)
BACKBONES = [dict(depth=depth, num_stages=ns, strides=(1, 2, 2, 2)[:ns], dilations=(1, 1, 1, 1)[:ns], out_indices=(ns - 1,), style=style, norm_cfg=GN)
             for depth in (50, 101) for ns in (3, 4) for style in ('pytorch', 'caffe')]
HEADS = [dict(depth=101, stage=3, stride=1, dilation=2, external_conv=True, norm_cfg=GN)]
BLOCK = dict(inplanes=128, planes=32, norm_cfg=dict(type='GN', num_groups=8))     # GroupNorm(8, 32) and GroupNorm(8, 128): 4 and 16 channels per group
BLOCK_INPUT = (2, 128, 9, 11)


def randomise(module, g):
    """Weights of the size a trained net has, gamma and beta away from the identity."""
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g, dtype=torch.float64) / fan ** 0.5
        elif isinstance(m, nn.GroupNorm):
            n = m.weight.shape[0]
            m.weight.data = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
            m.bias.data = torch.randn(n, generator=g, dtype=torch.float64) * 0.2


def main():
    MG.install_reference()
    rn = sys.modules['mmdet.models.backbones.resnet']
    rl = sys.modules['mmdet.models.shared_heads.res_layer']
    cases = []
    for kw in BACKBONES:
        cases.append(dict(cls='ResNet', kwargs=RX.listed(kw), runs=RX.keys_of(rn.ResNet(**kw))))
        print('ResNet %s: %d runs' % (kw, len(cases[-1]['runs'])))
    for kw in HEADS:
        cases.append(dict(cls='ResLayer', kwargs=RX.listed(kw), runs=RX.keys_of(rl.ResLayer(**kw))))
        print('ResLayer %s: %d runs' % (kw, len(cases[-1]['runs'])))
    path = os.path.join(MG.OUT, 'gn_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/backbones/resnet.py', 'mmdet/models/shared_heads/res_layer.py', 'mmdet/models/utils/norm.py'],
                       suffixes=RX.SUFFIXES, templates=RX.TEMPLATES, cases=cases), f, sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    g = torch.Generator().manual_seed(25)
    x = torch.randn(BLOCK_INPUT, generator=g, dtype=torch.float64)
    arrays = dict(x=x)
    # a: pytorch style, stride 2 on the 3x3, with the projection shortcut (conv, GroupNorm); b: an identity block at dilation 2 (4 planes == inplanes)
    down = nn.Sequential(nn.Conv2d(BLOCK['inplanes'], 4 * BLOCK['planes'], 1, stride=2, bias=False), nn.GroupNorm(8, 4 * BLOCK['planes']))
    blocks = dict(a=rn.Bottleneck(stride=2, dilation=1, downsample=down, style='pytorch', **BLOCK),
                  b=rn.Bottleneck(stride=1, dilation=2, downsample=None, style='pytorch', **BLOCK))
    for name, blk in blocks.items():
        blk = blk.double().eval()
        randomise(blk, g)
        with torch.no_grad():
            y = blk(x)
        assert y.dtype == torch.float64 and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
        for k, v in blk.state_dict().items():
            arrays['%s.%s' % (name, k)] = v
        arrays['%s.out' % name] = y
        print('block %s: out %s, |out| max %.3f' % (name, tuple(y.shape), float(y.abs().max())))
    MG.save('g25_gn_block', **arrays)


if __name__ == '__main__':
    main()
