"""Generates tests/golden/resnext_modules.json and tests/golden/g21_resnext_block.npz by running the REFERENCE's own ResNeXt code
(build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_resnext_golden.py

mmdet/models/backbones/resnext.py and mmdet/models/shared_heads/resx_layer.py are loaded where they lie on top of make_golden.py's
stub loader (install_reference, `_load`).  resnext_modules.json holds, per constructor call, the keywords and the state-dict keys
with their shapes, in order -- stored without loss as runs of consecutive blocks of a stage (or '' for the stem) that share one
form, each run naming an entry of shared tables of key suffixes and shapes, because a net repeats a few block forms dozens of times; g21_resnext_block.npz holds two of the reference's resnext.Bottleneck blocks in float64 (randomised weights and
BatchNorm statistics, eval mode), their parameters, one input and their outputs.  Nothing of the reference is copied: the script
executes it and stores names and numbers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

BACKBONES = [dict(depth=depth, groups=groups, base_width=4, num_stages=ns, strides=(1, 2, 2, 2)[:ns], dilations=(1, 1, 1, 1)[:ns],
                  out_indices=(ns - 1,), style=style)
             for depth in (50, 101) for groups in (32, 64) for ns in (3, 4) for style in ('pytorch', 'caffe')]
HEADS = [dict(depth=101, stage=3, stride=1, dilation=2, groups=32, base_width=4, external_conv=True)]
BLOCK = dict(inplanes=128, planes=32, groups=8, base_width=16)        # width 64, 8 channels per group
BLOCK_INPUT = (2, 128, 9, 11)


def load_reference():
    MG.install_reference()
    bb = sys.modules['mmdet.models.backbones']
    rx = MG._load('mmdet.models.backbones.resnext', 'mmdet/models/backbones/resnext.py')
    bb.ResNeXt, bb.make_resx_layer = rx.ResNeXt, rx.make_res_layer
    rxl = MG._load('mmdet.models.shared_heads.resx_layer', 'mmdet/models/shared_heads/resx_layer.py')
    return rx, rxl


SUFFIXES, TEMPLATES = [], []      # the shared tables: lists of key suffixes, and [index into SUFFIXES, the shapes in that order]


def _index(table, item):
    if item not in table:
        table.append(item)
    return table.index(item)


def keys_of(module):
    """The state dict's ordered (key, shape) list as runs [stage ('layer2' or ''), first block, blocks, index into TEMPLATES]: `blocks`
    consecutive blocks of the stage that share one (suffixes, shapes) form (tests/test_gconv_refs.py: _expand undoes it)."""
    blocks = []
    for k, v in module.state_dict().items():
        parts = k.split('.')
        n = 2 if parts[0].startswith('layer') else 0
        prefix, suffix = '.'.join(parts[:n]), '.'.join(parts[n:])
        if not blocks or blocks[-1][0] != prefix:
            blocks.append((prefix, [], []))
        blocks[-1][1].append(suffix)
        blocks[-1][2].append(list(v.shape))
    runs = []
    for prefix, suffixes, shapes in blocks:
        stage, _, idx = prefix.partition('.')
        t = _index(TEMPLATES, [_index(SUFFIXES, suffixes), shapes])
        if runs and runs[-1][0] == stage and runs[-1][3] == t and idx and runs[-1][1] + runs[-1][2] == int(idx):
            runs[-1][2] += 1
        else:
            runs.append([stage, int(idx or 0), 1, t])
    return runs


def listed(kw):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}


def randomise(module, g):
    """Weights of the size a trained net has and BatchNorm statistics away from the identity, so that no term of the folded form drops out."""
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g, dtype=torch.float64) / fan ** 0.5
        elif isinstance(m, nn.BatchNorm2d):
            n = m.weight.shape[0]
            m.weight.data = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
            m.bias.data = torch.randn(n, generator=g, dtype=torch.float64) * 0.2
            m.running_mean.data = torch.randn(n, generator=g, dtype=torch.float64) * 0.2
            m.running_var.data = torch.rand(n, generator=g, dtype=torch.float64) + 0.5


def main():
    rx, rxl = load_reference()
    cases = []
    for kw in BACKBONES:
        cases.append(dict(cls='ResNeXt', kwargs=listed(kw), runs=keys_of(rx.ResNeXt(**kw))))
        print('ResNeXt %s: %d runs' % (kw, len(cases[-1]['runs'])))
    for kw in HEADS:
        cases.append(dict(cls='ResXLayer', kwargs=listed(kw), runs=keys_of(rxl.ResXLayer(**kw))))
        print('ResXLayer %s: %d runs' % (kw, len(cases[-1]['runs'])))
    path = os.path.join(MG.OUT, 'resnext_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/backbones/resnext.py', 'mmdet/models/shared_heads/resx_layer.py'], suffixes=SUFFIXES, templates=TEMPLATES, cases=cases), f,
                  sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    g = torch.Generator().manual_seed(21)
    x = torch.randn(BLOCK_INPUT, generator=g, dtype=torch.float64)
    arrays = dict(x=x)
    # a: pytorch style, stride 2 on the 3x3, with the projection shortcut; b: an identity block at dilation 2 (4 planes == inplanes)
    down = nn.Sequential(nn.Conv2d(BLOCK['inplanes'], 4 * BLOCK['planes'], 1, stride=2, bias=False), nn.BatchNorm2d(4 * BLOCK['planes']))
    blocks = dict(a=rx.Bottleneck(stride=2, dilation=1, downsample=down, style='pytorch', **BLOCK),
                  b=rx.Bottleneck(stride=1, dilation=2, downsample=None, style='pytorch', **BLOCK))
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
    MG.save('g21_resnext_block', **arrays)


if __name__ == '__main__':
    main()
