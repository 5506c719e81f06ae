"""CPU tests of RoIPool: the statement of tests/roi_pool_refs.py against its own planted mistakes and against torch autograd, the
case generator's families, the registry, the module contract, the refusals that need no GPU, the C ABI's symbols and the training
entry points' refusal.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import hvrnet_amd
from hvrnet_amd import native, ops, registry
from hvrnet_amd.config import hvr_config, selsa_config
from hvrnet_amd.roi_extractor import SingleRoIExtractor
from tests import roi_pool_refs as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hvr_hip.h')


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize('mistake', R.FWD_MISTAKES)
def test_every_planted_forward_mistake_changes_a_value_or_an_argmax(mistake):
    changed = {}
    for name in ('c8', 'c64'):
        for (PH, PW) in R.OUT_SIZES:
            val, arg, _ = R.statement(name, PH, PW)
            bval, barg, _ = R.statement(name, PH, PW, mistake)
            changed[(name, PH, PW)] = int((val != bval).sum()) + int((arg != barg).sum())
    print(mistake, changed)
    assert sum(changed.values()) > 0, mistake
    assert changed[('c8', 7, 7)] > 0 or changed[('c64', 7, 7)] > 0, mistake


def test_the_planted_backward_mistake_changes_the_gradient():
    case = R.make_case('c8')
    _, arg, rec = R.statement('c8', 7, 7)
    assert (arg == -1).any()
    go = R.grad_out_ints(arg.shape, 3)
    good = R.backward_statement(go, case['rois'], arg, R.B, R.H, R.W)[0]
    bad = R.backward_statement(go, case['rois'], arg, R.B, R.H, R.W, mistake='minus1_to_0')[0]
    assert (good != bad).any() and (good[:, 0, 0] != bad[:, 0, 0]).any()
    for fam in ('malformed_x', 'batch_minus', 'batch_past', 'off_left'):
        k = case['family'][fam]
        only = np.zeros_like(go)
        only[k] = go[k]
        assert not R.backward_statement(only, case['rois'], arg, R.B, R.H, R.W)[0].any(), fam


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_generated_cases_hold_their_families(name):
    case = R.make_case(name)
    C, K, constant = R.CASES[name]
    assert case['feat'].shape == (R.B, R.H, R.W, C) and case['rois'].shape == (K, 5) and case['rois'].dtype == np.float32
    assert case['feat'].max() < 0 and len(np.unique(case['feat'])) <= len(R.LEVELS)
    for dt in (torch.bfloat16, torch.float16, torch.float32):   # the values are the same numbers in every dtype
        assert torch.equal(torch.from_numpy(case['feat']).to(dt).double(), torch.from_numpy(case['feat']))
    R.check_families(case)
    want = set(R.WIDE_PICK) if name == 'wide' else {p[0] for p in R.prescribed_rois()}
    assert set(case['family']) == want
    for (PH, PW) in R.OUT_SIZES:
        val, arg, rec = R.statement(name, PH, PW)
        assert (rec['ties'][~rec['empty']] >= 1).all() and (rec['ties'] > 1).any()      # ties exist: "first" is tested
        assert ((arg == -1) == rec['empty'][..., None]).all() and (arg < R.H * R.W).all()
        assert (val[rec['empty']] == 0).all() and (val[~rec['empty']] < 0).all()        # a maximum started at 0 is wrong everywhere
        k = np.nonzero(~rec['empty'])[0][0]
        b = int(case['rois'][k][0])
        flat = case['feat'][b].reshape(R.H * R.W, C)
        ph, pw = np.nonzero(~rec['empty'][k])[0][0], np.nonzero(~rec['empty'][k])[1][0]
        assert (flat[arg[k, ph, pw], np.arange(C)] == val[k, ph, pw]).all()
    if constant:   # a constant frame: every pixel ties, the argmax is the bin's first pixel
        _, arg, rec = R.statement(name, 7, 7)
        ks = [k for k in range(K) if case['rois'][k][0] == 1 and not rec['empty'][k].all()]
        assert ks
        for k in ks:
            _, _, xe, ye = R.roi_geometry(case['rois'][k], R.B, R.H, R.W, 7, 7, R.SCALE)
            for ph in range(7):
                for pw in range(7):
                    if not rec['empty'][k, ph, pw]:
                        assert (arg[k, ph, pw] == ye[ph][0] * R.W + xe[pw][0]).all()
                        assert (rec['ties'][k, ph, pw] == rec['area'][k, ph, pw]).all()


def test_contraction_sensitive_rois_have_the_stated_last_bins():
    want = {(-39.0, 31.0): ((1, 2), (1, 3)), (-39.0, 95.0): ((4, 6), (4, 7)), (-37.0, 15.0): ((0, 1), (0, 2))}
    for (x1, x2), (stated, fused) in want.items():
        roi = np.array([0, x1, 16, x2, 111], dtype=np.float32)
        assert R.roi_geometry(roi, R.B, R.H, R.W, 7, 7, R.SCALE)[2][-1] == stated
        assert R.roi_geometry(roi, R.B, R.H, R.W, 7, 7, R.SCALE, contracted=True)[2][-1] == fused
        roi = np.array([0, 16, x1, 143, x2], dtype=np.float32)
        assert R.roi_geometry(roi, R.B, R.H, R.W, 7, 7, R.SCALE)[3][-1] == stated
        assert R.roi_geometry(roi, R.B, R.H, R.W, 7, 7, R.SCALE, contracted=True)[3][-1] == fused


@pytest.mark.parametrize('name', ['c8', 'c64'])
def test_backward_statement_equals_autograd_through_a_gather(name):
    case = R.make_case(name)
    C = case['C']
    for (PH, PW) in R.OUT_SIZES:
        val, arg, rec = R.statement(name, PH, PW)
        feat = torch.from_numpy(case['feat']).clone().requires_grad_(True)                       # f64
        go = torch.from_numpy(R.grad_out_normal(arg.shape, 7))
        flat = feat.reshape(R.B, R.H * R.W, C)
        a = torch.from_numpy(arg.astype(np.int64))
        frames = torch.from_numpy(case['rois'][:, 0].astype(np.int64)).clamp(0, R.B - 1)
        picked = torch.gather(flat[frames], 1, a.clamp(min=0).reshape(case['K'], PH * PW, C)).reshape(arg.shape)
        picked = torch.where(a >= 0, picked, torch.zeros((), dtype=torch.float64))
        assert torch.equal(picked.detach(), torch.from_numpy(val))
        (picked * go).sum().backward()
        g, n, sabs = R.backward_statement(go.numpy(), case['rois'], arg, R.B, R.H, R.W)
        assert np.abs(g - feat.grad.numpy()).max() <= 1e-13 * max(1.0, np.abs(g).max())
        assert n.sum() == int((arg >= 0).sum()) and (g[n == 0] == 0).all() and (sabs >= np.abs(g) - 1e-12).all() and n.max() > 1


# ------------------------------------------------------------------------------------------------ the module contract
def test_the_extractor_builds_roi_pool_by_name():
    ext = SingleRoIExtractor(roi_layer=dict(type='RoIPool', out_size=7), out_channels=256, featmap_strides=[16])
    layer = ext.roi_layers[0]
    assert isinstance(layer, ops.RoIPool) and layer.out_size == (7, 7) and layer.spatial_scale == 1 / 16 and layer.use_torchvision is False
    assert hvrnet_amd.RoIPool is ops.RoIPool and hvrnet_amd.roi_pool is ops.roi_pool and ops.roi_pool == ops.RoIPoolFunction.apply
    assert 'RoIPool(out_size, spatial_scale, use_torchvision=False)' in ops.__doc__


def test_repr_has_the_references_format():
    assert repr(ops.RoIPool(7, 1 / 16)) == 'RoIPool(out_size=(7, 7), spatial_scale=0.0625, use_torchvision=False)'
    assert repr(ops.RoIPool((2, 3), 0.125)) == 'RoIPool(out_size=(2, 3), spatial_scale=0.125, use_torchvision=False)'


def test_torchvision_and_cpu_tensors_are_refused():
    with pytest.raises(NotImplementedError):
        ops.RoIPool(7, 1 / 16, use_torchvision=True)
    data, rois = torch.zeros((1, 8, 5, 5)), torch.tensor([[0, 0.0, 0.0, 30.0, 30.0]])
    with pytest.raises(NotImplementedError):
        ops.RoIPool(3, 1 / 16)(data, rois)
    with pytest.raises(NotImplementedError):
        ops.roi_pool(data, rois, 3, 1 / 16)
    with pytest.raises(NotImplementedError):
        native.roi_pool_fwd(data.permute(0, 2, 3, 1).contiguous(), rois, 3, 3, 1 / 16)
    with pytest.raises(NotImplementedError):
        native.roi_pool_bwd(torch.zeros((1, 3, 3, 8)), rois, torch.zeros((1, 3, 3, 8), dtype=torch.int32), (1, 5, 5, 8))


def test_the_symbols_are_bound_declared_and_exported():
    header = open(HEADER).read()
    lib = _lib()
    for name, nargs in (('hvr_roi_pool_fwd', 14), ('hvr_roi_pool_bwd', 12)):
        assert name in native.SYMBOLS and len(native.SYMBOLS[name][1]) == nargs
        decl = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert decl and len(decl.group(1).split(',')) == nargs, name
        assert getattr(lib, name) is not None
    assert lib.hvr_abi_version() == 7 and native.ABI_VERSION == 7
    for word in ('FIRST pixel', 'argmax -1', 'no fused multiply-add', 'before the conversion to int'):
        assert word in header, word


# ------------------------------------------------------------------------------------------------ the training entry points
def _build(builtin, roi_layer):
    cfg = builtin()
    cfg.model.bbox_roi_extractor['roi_layer'] = dict(roi_layer)
    return registry.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('builtin', [selsa_config, hvr_config])
def test_training_accepts_roi_pool_and_still_refuses_the_deformable_packs(builtin):
    model = _build(builtin, dict(type='RoIPool', out_size=7))
    layer = model._train_roi_layer()
    assert isinstance(layer, ops.RoIPool) and layer is model.bbox_roi_extractor.roi_layers[0]
    assert isinstance(_build(builtin, dict(type='RoIAlign', out_size=7, sample_num=2))._train_roi_layer(), ops.RoIAlign)
    assert set(model.state_dict()) == set(_build(builtin, dict(type='RoIAlign', out_size=7, sample_num=2)).state_dict())   # no parameters
    pack = _build(builtin, dict(type='DeformRoIPoolingPack', out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1,
                                deform_fc_channels=64))
    with pytest.raises(NotImplementedError) as e:
        pack._train_roi_layer()
    assert str(e.value) == 'training runs through RoIAlign only: roi_layer DeformRoIPoolingPack is inference only (it has no backward)'
    with pytest.raises(NotImplementedError, match='DeformRoIPoolingPack'):
        pack.forward_train(None, None, None, None)
