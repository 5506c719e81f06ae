"""Generates tests/golden/dpool_modules.json by constructing the REFERENCE's own deformable RoI pooling modules (build container
only; needs the reference tree at make_golden.REF):

    python tests/golden/make_dpool_golden.py

mmdet/ops/dcn/deform_pool.py is loaded where it lies on top of make_golden.py's stub loader (`_pkg`, `_load`), beside an empty
stand-in for its compiled extension (never called: nothing is pooled here).  The fixture holds, per constructor call, the
arguments, the state-dict keys with their shapes, which tensors start at zero, and the plain attributes of the module.  Nothing
of the reference is copied: the script executes it and stores names and numbers.
"""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402

CASES = [   # class, constructor keywords (as a config's roi_layer would give them, + spatial_scale from the extractor)
    ('DeformRoIPooling', dict(spatial_scale=1 / 16, out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1)),
    ('DeformRoIPoolingPack', dict(spatial_scale=1 / 16, out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1)),
    ('DeformRoIPoolingPack', dict(spatial_scale=1 / 16, out_size=7, out_channels=256, no_trans=True)),
    ('DeformRoIPoolingPack', dict(spatial_scale=1 / 8, out_size=3, out_channels=64, no_trans=False, part_size=3, sample_per_part=2,
                                  trans_std=0.05, num_offset_fcs=2, deform_fc_channels=128)),
    ('ModulatedDeformRoIPoolingPack', dict(spatial_scale=1 / 16, out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1)),
    ('ModulatedDeformRoIPoolingPack', dict(spatial_scale=1 / 16, out_size=(5, 5), out_channels=32, no_trans=False, num_offset_fcs=1,
                                           num_mask_fcs=3, deform_fc_channels=64)),
    ('ModulatedDeformRoIPoolingPack', dict(spatial_scale=1 / 16, out_size=7, out_channels=256, no_trans=True)),
]
ATTRS = ('spatial_scale', 'out_size', 'out_channels', 'no_trans', 'group_size', 'part_size', 'sample_per_part', 'trans_std',
         'num_offset_fcs', 'num_mask_fcs', 'deform_fc_channels')


def load_reference_module():
    MG._pkg('mmdet', os.path.join(MG.REF, 'mmdet'))
    MG._pkg('mmdet.ops')
    MG._pkg('mmdet.ops.dcn', os.path.join(MG.REF, 'mmdet/ops/dcn'))
    ext = types.ModuleType('mmdet.ops.dcn.deform_pool_cuda')
    sys.modules['mmdet.ops.dcn.deform_pool_cuda'] = ext
    sys.modules['mmdet.ops.dcn'].deform_pool_cuda = ext
    return MG._load('mmdet.ops.dcn.deform_pool', 'mmdet/ops/dcn/deform_pool.py')


def describe(module):
    sd = module.state_dict()
    out = dict(keys=[[k, list(v.shape)] for k, v in sd.items()], zero=[k for k, v in sd.items() if not bool(v.any())], attrs={})
    for a in ATTRS:
        if hasattr(module, a):
            v = getattr(module, a)
            out['attrs'][a] = list(v) if isinstance(v, tuple) else v
    return out


def main():
    ref = load_reference_module()
    cases = []
    for name, kw in CASES:
        d = describe(getattr(ref, name)(**kw))
        d.update(cls=name, kwargs={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})
        cases.append(d)
        print('%s %s: %d tensors, %d start at zero' % (name, kw, len(d['keys']), len(d['zero'])))
    path = os.path.join(MG.OUT, 'dpool_modules.json')
    with open(path, 'w') as f:
        json.dump(dict(source='mmdet/ops/dcn/deform_pool.py', cases=cases), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s' % path)


if __name__ == '__main__':
    main()
