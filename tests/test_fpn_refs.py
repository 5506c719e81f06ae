"""CPU tests of the multi-level feature path: the statements of tests/fpn_refs.py against the fixtures the reference wrote
(tests/golden/g27_fpn.npz, fpn_modules.json), the level rule against torch's own evaluation, and the host surface (constructor,
state-dict keys, refusals, registry, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import native, registry
from hvrnet_amd.necks import FPN
from hvrnet_amd.roi_extractor import SingleRoIExtractor
from tests import fpn_refs as R

NEW_SYMBOLS = ['hvr_fpn_merge_supported', 'hvr_fpn_merge', 'hvr_roi_align_levels_supported', 'hvr_roi_align_levels_fwd']


@pytest.fixture(scope='module')
def gold():
    return R.golden()


@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_the_f64_statement_reproduces_the_reference(gold, name):
    """fpn_forward on the stored inputs and weights equals the reference's f64 outputs to 1e-12 relative."""
    got = R.fpn_forward(R.fixture_inputs(gold), R.fixture_weights(gold, name), R.CONFIGS[name])
    err = R.rel_err(got, R.fixture_outs(gold, name))
    print('fpn_forward %s: relative error %.3g' % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize('name,mistake', [('faster', 'bilinear'), ('faster', 'add_level_off'), ('faster', 'offset1'), ('retina', 'bilinear'),
                                          ('retina', 'extra_on_outs'), ('relu3', 'add_level_off')])
def test_planted_mistakes_leave_the_bound(gold, name, mistake):
    """Each wrong reading of fpn.py:101-141 misses the reference by orders of magnitude more than 1e-12."""
    got = R.fpn_forward(R.fixture_inputs(gold), R.fixture_weights(gold, name), R.CONFIGS[name], mistake=mistake)
    err = R.rel_err(got, R.fixture_outs(gold, name))
    print('fpn_forward %s with %s: relative error %.3g' % (name, mistake, err))
    assert err > 1e-6


def test_the_level_rule_equals_the_stored_levels(gold):
    rois, levels = gold['ext.rois'], gold['ext.levels']
    assert np.array_equal(R.level_rule(rois, 56, 4), levels)
    assert set(levels.tolist()) == {0, 1, 2, 3} and not np.isnan(rois).any()
    b = R.boundary_boxes()
    want = [0, 1, 2, 3, 0, 1, 2, 2]    # a square of side 56 * 2^k is on level k; 112 x 111 is just under 112, 111 x 113 and 223 x 225 just over
    rois5 = np.concatenate([np.zeros((len(b), 1), np.float32), b], 1)
    assert R.level_rule(rois5, 56, 4).tolist() == R.torch_levels(rois5, 56, 4).tolist()
    assert R.level_rule(rois5, 56, 4).tolist()[:4] == want[:4]
    nan = np.array([[0, 10, 10, 5, 30]], np.float32)      # one side negative: sqrt of a negative product
    assert R.level_rule(nan, 56, 4).tolist() == [0]
    both = np.array([[0, 10, 10, 5, 5]], np.float32)      # both sides negative: a positive product, an ordinary level
    assert R.level_rule(both, 56, 4).tolist() == R.torch_levels(both, 56, 4).tolist()
    for L in (1, 2, 3):
        assert np.array_equal(R.level_rule(rois, 56, L), np.minimum(levels, L - 1))


def test_the_level_rule_against_torch_on_random_boxes():
    """2 000 000 seeded boxes: the comparison rule differs from torch's floor(log2()) in at most a share of 1e-5 (it can differ only
    where log2f rounds a value just below a power of two up to it)."""
    g = torch.Generator().manual_seed(2027)
    n = 2000000
    xy = torch.rand((n, 2), generator=g) * 1000
    wh = torch.exp(torch.rand((n, 2), generator=g) * float(np.log(1200.0)))
    rois = torch.cat([torch.zeros((n, 1)), xy, xy + wh], 1).numpy()
    a, b = R.level_rule(rois, 56, 4), R.torch_levels(rois, 56, 4)
    share = float((a != b).mean())
    print('level rule vs torch floor(log2()): %d of %d differ (share %.3g), levels %s' % (int((a != b).sum()), n, share, np.bincount(a).tolist()))
    assert share <= 1e-5 and np.bincount(a, minlength=4).min() > n // 100
    ints = np.round(rois)
    assert float((R.level_rule(ints, 56, 4) != R.torch_levels(ints, 56, 4)).mean()) <= 1e-5


def test_constructor_and_state_dict_equal_the_reference():
    for case in R.modules()['cases']:
        m = FPN(**case['kwargs'])
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == case['keys'], case['name']
        assert case['kwargs'] == R.CONFIGS[case['name']]
    import inspect
    sig = inspect.signature(FPN.__init__)
    assert list(sig.parameters)[1:] == ['in_channels', 'out_channels', 'num_outs', 'start_level', 'end_level', 'add_extra_convs',
                                        'extra_convs_on_inputs', 'relu_before_extra_convs', 'no_norm_on_lateral', 'conv_cfg', 'norm_cfg',
                                        'activation']
    m = FPN([32, 64], 32, 2)
    m.init_weights()
    for k, v in m.state_dict().items():
        if k.endswith('bias'):
            assert float(v.abs().max()) == 0.0
        else:
            fan_in, fan_out = v.shape[1] * v.shape[2] * v.shape[3], v.shape[0] * v.shape[2] * v.shape[3]
            assert 0.5 < float(v.abs().max()) / np.sqrt(6.0 / (fan_in + fan_out)) <= 1.0, k       # xavier-uniform, gain 1


def test_every_refusal_names_its_argument():
    with pytest.raises(NotImplementedError, match='conv_cfg'):
        FPN([32, 64], 32, 2, conv_cfg=dict(type='ConvWS'))
    with pytest.raises(NotImplementedError, match='norm_cfg'):
        FPN([32, 64], 32, 2, norm_cfg=dict(type='BN'))
    with pytest.raises(NotImplementedError, match='activation'):
        FPN([32, 64], 32, 2, activation='leaky_relu')
    ext = SingleRoIExtractor(dict(type='RoIPool', out_size=7), 32, [4, 8])
    with pytest.raises(NotImplementedError, match='RoIPool'):
        ext([torch.zeros(1, 32, 8, 8), torch.zeros(1, 32, 4, 4)], torch.zeros(1, 5))
    with pytest.raises(native.HvrError, match='route'):
        native.roi_align_levels([torch.zeros(1, 4, 4, 8)], torch.zeros(1, 5), 7, [0.25], route='fast')
    with pytest.raises(native.HvrError, match='scales'):
        native.roi_align_levels([torch.zeros(1, 4, 4, 8)], torch.zeros(1, 5), 7, [0.25, 0.125])


def test_cpu_tensors_raise_gpu_only():
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.fpn_merge([torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)])
    with pytest.raises(NotImplementedError, match='GPU only'):
        native.roi_align_levels([torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)], torch.zeros(1, 5), 7, [0.25, 0.125])
    with pytest.raises(NotImplementedError, match='GPU only'):
        FPN([32, 64], 32, 2)([torch.zeros(1, 32, 4, 4), torch.zeros(1, 64, 2, 2)])
    ext = SingleRoIExtractor(dict(type='RoIAlign', out_size=7, sample_num=2), 32, [4, 8])
    with pytest.raises(NotImplementedError, match='GPU only'):
        ext([torch.zeros(1, 32, 8, 8), torch.zeros(1, 32, 4, 4)], torch.zeros(1, 5))


def test_registry_builds_the_neck_and_a_detector_with_it():
    neck = registry.build_neck(dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5))
    assert isinstance(neck, FPN) and hvrnet_amd.FPN is FPN and registry.NECKS.get('FPN') is FPN and hvrnet_amd.build_neck is registry.build_neck
    from hvrnet_amd.config import selsa_config
    from hvrnet_amd.detectors import TwoStageDetector
    c = selsa_config()
    model = dict(c.model, neck=dict(type='FPN', in_channels=[1024], out_channels=256, num_outs=1))
    det = registry.build_detector(model, train_cfg=c.get('train_cfg'), test_cfg=c.get('test_cfg'))
    assert det.with_neck and isinstance(det.neck, FPN)
    assert any(k.startswith('neck.lateral_convs.0.conv.') for k in det.state_dict())
    with pytest.raises(NotImplementedError, match='neck'):      # the training entry points refuse a detector with a neck by name
        det._train_roi_layer()
    with pytest.raises(NotImplementedError, match='neck'):
        det.forward_train_sampled(None, None, None, None, None, None, None)
    two = TwoStageDetector(backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch'),
                           neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
                           bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', out_size=7, sample_num=2),
                                                   out_channels=256, featmap_strides=[4, 8, 16, 32]))
    assert two.with_neck and two.neck.num_outs == 5
    with pytest.raises(NotImplementedError, match='mask_head'):
        TwoStageDetector(backbone=dict(type='ResNet', depth=50), mask_head=dict(type='FCNMaskHead'))


def test_exports_are_declared_bound_and_present():
    header = open(native.HEADER_PATH).read()
    capi = open(os.path.join(os.path.dirname(native.LIB_PATH), 'csrc', 'capi.hip')).read()
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.lib()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b%s\(' % sym, header), '%s is not declared in include/hvr_hip.h' % sym
        assert re.search(r'\b%s\(' % sym, capi), '%s is not defined in capi.hip' % sym
        assert sym in native.SYMBOLS and hasattr(lib, sym), sym
    assert lib.hvr_abi_version() == native.ABI_VERSION == 7
    for word in ('rounded to `dtype` ONCE', 'log2f rounds a value just below a power of two up to it', 'level 0', 'bit for bit'):
        assert word in header, word
    assert ctypes.sizeof(native.RoiLevelsDesc) == 152
    # the instance sets: the queries need no device
    for C in range(64, 1025, 64):
        for dt in (native.HVR_F32, native.HVR_BF16, native.HVR_F16):
            assert lib.hvr_fpn_merge_supported(4, C, dt) == 1 and lib.hvr_roi_align_levels_supported(4, C, dt) == 1
    assert lib.hvr_fpn_merge_supported(4, 12, native.HVR_F32) == 1 and lib.hvr_fpn_merge_supported(4, 12, native.HVR_BF16) == 0
    assert lib.hvr_fpn_merge_supported(5, 64, native.HVR_F32) == 0 and lib.hvr_fpn_merge_supported(4, 64, native.HVR_F16S) == 0
    assert lib.hvr_roi_align_levels_supported(4, 24, native.HVR_BF16) == 1 and lib.hvr_roi_align_levels_supported(4, 6, native.HVR_F32) == 0
    units = [line.split('#')[0].split() for line in open(os.path.join(os.path.dirname(native.LIB_PATH), 'csrc', 'units.txt'))]
    assert ['fpn', 'remarks'] in units
