"""Generates tests/golden/gen_attention_modules.json and tests/golden/g24_gen_attention.npz by running the REFERENCE's own generalized
attention block, and tests/golden/g24_gen_attention_blocks.npz (build container only; needs the reference tree at make_golden.REF):

    python tests/golden/make_gen_attention_golden.py

mmdet/models/plugins/generalized_attention.py is loaded where it lies on top of make_golden.py's stub loader, and the real class is
assigned over the dummy `GeneralizedAttention` the loader left in the loaded resnet module.  Three process-local patches, of the kind
make_golden.py lists for other defects of the reference (nothing outside this process changes):
  * the stub mmcv.cnn.kaiming_init gains the `a` and `distribution='uniform'` arguments the block's init_weights passes;
  * get_position_embedding calls .cuda(device) on every tensor it makes: torch.Tensor.cuda is the identity here (a CPU run);
  * it builds its tables in the DEFAULT dtype: the default dtype is float64 during the float64 evaluation, float32 during the float32 one.
gen_attention_modules.json holds, per constructor call, the keywords and the state-dict keys with their shapes in order (the run-length
form of resnext_modules.json, make_resnext_golden.keys_of) for ResNet-50 / -101 with attention blocks in layers 3 and 4, and for the bare
module one entry per attention type in scope.  g24_gen_attention.npz holds, in float64 (randomised weights, biases, gamma and BatchNorm
statistics, eval mode -- the reference starts gamma at 0, which makes a fresh block the identity):
  a.*  GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='1111') on a.x [2,64,5,7];
  b.*  the same with '0010' (the saliency shortcut);     c.*  with '0011';
  d.*  GeneralizedAttention(72, num_heads=9, kv_stride=1, attention_type='1001') on d.x [1,72,6,5]        (d = 8);
  e.*  GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='1011', position_embedding_dim=32, position_magnitude=2) on [2,64,6,5];
  f.*  an identity Bottleneck(256, 64, gen_attention=dict(num_heads=4, kv_stride=2)) on f.x [2,256,6,9]      (d = 16);
  g.*  a projection Bottleneck(64, 32, stride=2) with gen_attention (2 heads, kv_stride 2, '0111') AND gcb on g.x [2,64,9,11] (odd sides).
Parameters and inputs are drawn in float32 and widened for the float64 run; every one of them is a float32 value and is STORED as float32
(asserted), which keeps each file under the size limit of a committed file: a.* .. e.* are in g24_gen_attention.npz, f.* and g.* in
g24_gen_attention_blocks.npz.  `*.out` is the float64 evaluation (stored as float64), `*.out_f32` the reference's own float32 evaluation of
the same module; the maker prints their distance, which tests/test_gen_attention_refs.py scales into its bound.  Nothing of the reference is copied: the script executes it
and stores names and numbers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402
from tests.golden import make_resnext_golden as RXG  # noqa: E402
from tests.golden import make_gcb_golden as GCG  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

GA = dict(spatial_range=-1, num_heads=8, attention_type='1111', kv_stride=2)
SWA = ((), (), (0, 2, 5), (0, 1, 2))
TYPES = ('1000', '0010', '0001', '1010', '1001', '0011', '1011', '0101', '0111', '1101', '1111')


def load_reference():
    rn, rx, cbm = GCG.load_reference()
    cnn = sys.modules['mmcv.cnn']

    def kaiming_init(module, a=0, mode='fan_out', nonlinearity='relu', bias=0, distribution='normal'):   # mmcv/cnn/weight_init.py
        assert distribution in ('uniform', 'normal')
        init = nn.init.kaiming_uniform_ if distribution == 'uniform' else nn.init.kaiming_normal_
        init(module.weight, a=a, mode=mode, nonlinearity=nonlinearity)
        if getattr(module, 'bias', None) is not None:
            nn.init.constant_(module.bias, bias)
    cnn.kaiming_init = kaiming_init
    torch.Tensor.cuda = lambda self, *a, **k: self
    gam = MG._load('mmdet.models.plugins.generalized_attention', 'mmdet/models/plugins/generalized_attention.py')
    rn.GeneralizedAttention = sys.modules['mmdet.models.plugins'].GeneralizedAttention = gam.GeneralizedAttention
    return rn, gam


def randomise32(module, g):
    """make_gcb_golden.randomise32, plus gamma, the two biases and the fc weights of every attention block (float32 values)."""
    GCG.randomise32(module, g)
    for m in module.modules():
        if type(m).__name__ == 'GeneralizedAttention':
            m.gamma.data = (torch.rand(1, generator=g) + 0.5).double()
            for name in ('appr_bias', 'geom_bias'):
                if hasattr(m, name):
                    p = getattr(m, name)
                    p.data = (torch.rand(p.shape, generator=g) * 2.0 - 1.0).double()
            for name in ('appr_geom_fc_x', 'appr_geom_fc_y'):
                if hasattr(m, name):
                    w = getattr(m, name).weight
                    w.data = ((torch.rand(w.shape, generator=g) * 2.0 - 1.0) * (3.0 / w.shape[1]) ** 0.5).double()


def evaluate(arrays, name, module, x, g):
    module = module.double().eval()
    randomise32(module, g)
    with torch.no_grad():
        torch.set_default_dtype(torch.float64)
        y = module(x)
        torch.set_default_dtype(torch.float32)
        y32 = module.float()(x.float())
    module.double()
    assert y.dtype == torch.float64 and y32.dtype == torch.float32 and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
    assert y.shape != x.shape or float((y - x).abs().max()) > 0.05, 'the block is the identity'
    for k, v in module.state_dict().items():
        assert not v.is_floating_point() or bool((v.float().double() == v).all())
        arrays['%s.%s' % (name, k)] = v.float() if v.is_floating_point() else v
    assert bool((x.float().double() == x).all())
    arrays['%s.x' % name], arrays['%s.out' % name], arrays['%s.out_f32' % name] = x.float(), y, y32
    print('%s: out %s, |out| max %.3f, f32 run off by %.3e' % (name, tuple(y.shape), float(y.abs().max()), float((y32.double() - y).abs().max())))


def main():
    rn, gam = load_reference()
    cases = []
    for depth in (50, 101):
        kw = dict(depth=depth, gen_attention=GA, stage_with_gen_attention=SWA)
        net = rn.ResNet(**kw)
        cases.append(dict(cls='ResNet', kwargs=GCG.listed(kw), runs=RXG.keys_of(net)))
        print('ResNet %d: %d runs, %d keys' % (depth, len(cases[-1]['runs']), len(net.state_dict())))
    bare = []
    for t in TYPES:
        kw = dict(in_dim=64, num_heads=8, kv_stride=2, attention_type=t)
        bare.append(dict(kwargs=kw, keys=[[k, list(v.shape)] for k, v in gam.GeneralizedAttention(**kw).state_dict().items()]))
    kw = dict(in_dim=72, attention_type='1011', position_embedding_dim=32)     # the default nine heads: d = 8
    bare.append(dict(kwargs=kw, keys=[[k, list(v.shape)] for k, v in gam.GeneralizedAttention(**kw).state_dict().items()]))
    path = os.path.join(MG.OUT, 'gen_attention_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source=['mmdet/models/plugins/generalized_attention.py', 'mmdet/models/backbones/resnet.py'],
                       suffixes=RXG.SUFFIXES, templates=RXG.TEMPLATES, cases=cases, bare=bare), f, sort_keys=True, indent=None, separators=(',', ':'))
        f.write('\n')
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))

    g = torch.Generator().manual_seed(24)
    arrays = {}
    x = lambda *s: torch.randn(s, generator=g).double()   # noqa: E731
    evaluate(arrays, 'a', gam.GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='1111'), x(2, 64, 5, 7), g)
    evaluate(arrays, 'b', gam.GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='0010'), x(2, 64, 5, 7), g)
    evaluate(arrays, 'c', gam.GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='0011'), x(2, 64, 5, 7), g)
    evaluate(arrays, 'd', gam.GeneralizedAttention(72, num_heads=9, kv_stride=1, attention_type='1001'), x(1, 72, 6, 5), g)
    evaluate(arrays, 'e', gam.GeneralizedAttention(64, num_heads=8, kv_stride=2, attention_type='1011', position_embedding_dim=32, position_magnitude=2),
             x(2, 64, 6, 5), g)
    evaluate(arrays, 'f', rn.Bottleneck(256, 64, gen_attention=dict(num_heads=4, kv_stride=2)), x(2, 256, 6, 9), g)
    down = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    evaluate(arrays, 'g', rn.Bottleneck(64, 32, stride=2, downsample=down, gen_attention=dict(num_heads=2, kv_stride=2, attention_type='0111'),
                                        gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))), x(2, 64, 9, 11), g)
    blocks = ('f.', 'g.')
    MG.save('g24_gen_attention', **{k: v for k, v in arrays.items() if not k.startswith(blocks)})
    MG.save('g24_gen_attention_blocks', **{k: v for k, v in arrays.items() if k.startswith(blocks)})


if __name__ == '__main__':
    main()
