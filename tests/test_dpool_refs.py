"""CPU checks of the deformable RoI pooling statement (tests/dpool_refs.py) and of the module surface (-m "not gpu"): an independent
scalar f32 evaluation of the rule inside the bound and equal on the exact families, every listed mistake outside the bound (or
unequal on an exact family), the case generator's coverage conditions, and the constructors / checkpoint / refusal contract of
DeformRoIPooling, DeformRoIPoolingPack and ModulatedDeformRoIPoolingPack."""
import json
import math
import os

import numpy as np
import pytest
import torch

from hvrnet_amd import ops, registry
from hvrnet_amd.config import hvr_config, selsa_config
from tests import dpool_refs as R
from tests import forward_kernel_refs as F

MODES = F.MODES
f32 = np.float32

# name -> generator keywords: A (the stock shape), B (parts != bins, two classes), C (position-sensitive groups)
CONFIGS = {
    'A': dict(B=2, H=9, W=11, out_channels=64, K=40, P=7, spp=4, ps=7),
    'B': dict(B=2, H=9, W=11, out_channels=32, K=24, P=3, spp=2, ps=2, ncls=2),
    'C': dict(B=2, H=9, W=11, out_channels=16, group_size=3, K=24, P=3, spp=4, ps=3),
}


def test_rnd_is_half_away_from_zero():
    x = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, -0.49999997, 3.0, -7.25, 8388607.5])
    want = torch.tensor([1.0, 2.0, 3.0, -1.0, -2.0, -3.0, 0.0, 0.0, 3.0, -7.0, 8388608.0])
    assert torch.equal(R.rnd(x), want)
    assert torch.equal(R.rnd(x), torch.tensor([float(np.float32(math.copysign(math.floor(abs(float(v)) + 0.5), float(v)))) for v in x]))
    assert not torch.equal(R.rnd(x, 'round_half_even'), want)


def _f32_rule(case, with_trans=True, with_mask=True):
    """The rule evaluated sample by sample with numpy float32 scalars (every operation rounded on its own), in the reference's
    summation order -- independent of the vectorised statement, positions included."""
    feat = case['feat'].float().numpy()
    rois = case['rois'].numpy().astype(f32)
    P, Cout, gs, ps, spp = case['P'], case['out_channels'], case['group_size'], case['part_size'], case['sample_per_part']
    s, tstd = f32(case['spatial_scale']), f32(case['trans_std'])
    trans = case['trans'].numpy().astype(f32) if (with_trans and case['trans'] is not None) else None
    mask = case['mask_logit'].numpy().astype(f32) if (with_mask and case['mask_logit'] is not None) else None
    B, H, W, C = feat.shape
    ncls = 1 if trans is None else trans.shape[1] // (2 * ps * ps)
    cpc = Cout // ncls
    out = np.zeros((rois.shape[0], P, P, Cout), f32)
    rnd = lambda v: f32(math.copysign(math.floor(abs(float(v)) + 0.5), float(v)))
    half = f32(0.5)
    for n, r in enumerate(rois):
        b = min(max(int(r[0]), 0), B - 1)
        sw, sh = f32(rnd(r[1]) * s) - half, f32(rnd(r[2]) * s) - half
        ew, eh = f32(f32(rnd(r[3]) + f32(1)) * s) - half, f32(f32(rnd(r[4]) + f32(1)) * s) - half
        rw, rh = max(f32(ew - sw), f32(0.1)), max(f32(eh - sh), f32(0.1))
        bw, bh = f32(rw / f32(P)), f32(rh / f32(P))
        subw, subh = f32(bw / f32(spp)), f32(bh / f32(spp))
        for ph in range(P):
            for pw in range(P):
                part_h = int(math.floor(f32(f32(f32(ph) / f32(P)) * f32(ps))))
                part_w = int(math.floor(f32(f32(f32(pw) / f32(P)) * f32(ps))))
                gw = min(max(int(math.floor(f32(f32(f32(pw) * f32(gs)) / f32(P)))), 0), gs - 1)
                gh = min(max(int(math.floor(f32(f32(f32(ph) * f32(gs)) / f32(P)))), 0), gs - 1)
                for cls in range(ncls):
                    tx = ty = f32(0)
                    if trans is not None:
                        t = trans[n].reshape(ncls, 2, ps, ps)
                        tx, ty = f32(t[cls, 0, part_h, part_w] * tstd), f32(t[cls, 1, part_h, part_w] * tstd)
                    wstart = f32(f32(f32(pw) * bw) + sw)
                    wstart = f32(wstart + f32(tx * rw))
                    hstart = f32(f32(f32(ph) * bh) + sh)
                    hstart = f32(hstart + f32(ty * rh))
                    ct = np.arange(cls * cpc, (cls + 1) * cpc)
                    c = (ct * gs + gh) * gs + gw
                    acc = np.zeros(cpc, f32)
                    count = 0
                    for ih in range(spp):
                        for iw in range(spp):
                            w = f32(wstart + f32(f32(iw) * subw))
                            h = f32(hstart + f32(f32(ih) * subh))
                            if w < -0.5 or w > W - 0.5 or h < -0.5 or h > H - 0.5:
                                continue
                            w, h = min(max(w, f32(0)), f32(W - 1)), min(max(h, f32(0)), f32(H - 1))
                            xl, xh, yl, yh = int(math.floor(w)), int(math.ceil(w)), int(math.floor(h)), int(math.ceil(h))
                            dx, dy = f32(w - f32(xl)), f32(h - f32(yl))
                            ox, oy = f32(f32(1) - dx), f32(f32(1) - dy)
                            v = (ox * oy) * feat[b, yl, xl, c] + (ox * dy) * feat[b, yh, xl, c]
                            v = v + (dx * oy) * feat[b, yl, xh, c]
                            v = v + (dx * dy) * feat[b, yh, xh, c]
                            acc = acc + v
                            count += 1
                    res = np.zeros(cpc, f32) if count == 0 else acc / f32(count)
                    if mask is not None:
                        with np.errstate(over='ignore'):                # (exp(128) = inf: the mask is then 0, as in f32 on the device)
                            res = res * f32(f32(1) / f32(f32(1) + np.exp(-mask[n, ph * P + pw], dtype=f32)))
                    out[n, ph, pw, cls * cpc:(cls + 1) * cpc] = res
    assert out.dtype == f32
    return torch.from_numpy(out)


SMALL = {
    'A': dict(B=2, H=6, W=7, out_channels=8, K=12, P=7, spp=4, ps=7),
    'B': dict(B=2, H=6, W=7, out_channels=8, K=12, P=3, spp=2, ps=2, ncls=2),
    'C': dict(B=2, H=6, W=7, out_channels=4, group_size=3, K=12, P=3, spp=3, ps=3),
}


@pytest.mark.parametrize('name', sorted(SMALL))
def test_scalar_f32_evaluation_lies_inside_the_bound(name):
    for mode in MODES:
        case = R.real_case(mode, seed=11, check=False, **SMALL[name])
        for with_trans, with_mask in ((True, True), (True, False), (False, False)):
            ref, bound = R.pool_statement(case['feat'], case['rois'], *R.args_of(case, with_trans, with_mask))
            got = _f32_rule(case, with_trans, with_mask).double()
            ratio, bad, _ = F.compare(got, ref - bound, ref + bound, ref)
            print('%s %s trans %d mask %d: worst |f32 - ref| / bound = %.3f' % (name, mode, with_trans, with_mask, ratio))
            assert bad == 0 and float(ref.abs().max()) > 0.3
            if mode != 'f32':
                lo, hi = R.stored_bracket(ref, bound, mode)
                assert F.compare(F.round_stored(got, mode), lo, hi, ref)[1] == 0


@pytest.mark.parametrize('family', R.EXACT_FAMILIES)
def test_exact_families_are_exact_in_f32(family):
    """On the exact families the independent scalar f32 evaluation EQUALS the statement."""
    mode = 'f16x2' if family == 'lo_act' else 'bf16'
    for (P, spp) in ((4, 2), (2, 4)):
        case = R.exact_case(mode, 8, family, H=6, W=7, out_channels=8, K=10, P=P, spp=spp)
        ref, _ = R.pool_statement(case['feat'], case['rois'], *R.args_of(case))
        ref = ref.float().double()      # (sigmoid(32) and sigmoid(-128) are 1 and 0 to f32 precision only)
        assert torch.equal(_f32_rule(case).double(), ref)
        if family == 'outside':
            assert not bool(ref.any())
        else:
            assert bool(ref.any())
        if family == 'zero':
            none, _ = R.pool_statement(case['feat'], case['rois'], None, *R.args_of(case)[1:])
            assert torch.equal(none.float().double(), ref)
        if family == 'lo_act':
            hi, lo = F.split_parts(ref, F.ACT_SCALE)
            assert bool((lo != 0).any())


def _config_for(mistake):
    if mistake in ('trans_by_bin', 'mask_by_part'):
        return 'B'
    if mistake == 'group_ignored':
        return 'C'
    return 'A'


@pytest.mark.parametrize('mistake', R.MISTAKES)
@pytest.mark.parametrize('mode', MODES)
def test_every_mistake_falls_outside_the_bound(mistake, mode):
    case = R.real_case(mode, seed=3, **CONFIGS[_config_for(mistake)])
    ref, bound = R.pool_statement(case['feat'], case['rois'], *R.args_of(case))
    lo, hi = R.stored_bracket(ref, bound, mode)
    wrong, _ = R.pool_statement(case['feat'], case['rois'], *R.args_of(case), mistake=mistake)
    stored = wrong if mode == 'f32' else F.round_stored(wrong.float().double(), mode)
    ratio, bad, _ = F.compare(stored, lo, hi, ref)
    right = ref if mode == 'f32' else F.round_stored(ref.float().double(), mode)
    assert F.compare(right, lo, hi, ref)[1] == 0                    # the statement itself passes ...
    print('%s %s: %d outside, worst / bracket = %.1f' % (mistake, mode, bad, ratio))
    assert bad > 0 and ratio > 10.0, (mistake, mode, bad, ratio)    # ... the mistake does not, by far


EXACT_MISTAKES = ('no_half_shift', 'roialign_border', 'no_edge_clamp', 'divide_by_spp2', 'trans_xy_swapped', 'trans_unscaled',
                  'mask_unapplied', 'batch_ignored')


@pytest.mark.parametrize('mistake', EXACT_MISTAKES)
def test_mistakes_are_unequal_on_an_exact_family(mistake):
    """(the remaining mistakes need what the exact families do not carry: corners on .5, a degenerate RoI, parts != bins, groups)"""
    case = R.exact_case('bf16', 4, 'eighths')
    ref, _ = R.pool_statement(case['feat'], case['rois'], *R.args_of(case))
    wrong, _ = R.pool_statement(case['feat'], case['rois'], *R.args_of(case), mistake=mistake)
    assert not torch.equal(F.round_stored(ref.float().double(), 'bf16'), F.round_stored(wrong.float().double(), 'bf16'))


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_generated_cases_carry_every_kind_of_bin_and_roi(name):
    case = R.real_case('f32', seed=5, **CONFIGS[name])                # (asserts its coverage itself)
    assert case['rois'].shape[0] == CONFIGS[name]['K']
    tame = dict(case)
    tame['rois'] = torch.tensor([[0, 32.0, 32.0, 96.0, 96.0]] * 4)    # RoIs inside the map only: the conditions must notice
    tame['trans'], tame['mask_logit'] = case['trans'][:4], None if case['mask_logit'] is None else case['mask_logit'][:4]
    with pytest.raises(AssertionError):
        R._assert_coverage(tame)


def test_bound_counts_the_roundings_of_the_rule():
    assert R.roundings(4, False) == 2 + 1 + 1 + 3 + 15 + 1 and R.roundings(2, True) == 2 + 1 + 1 + 3 + 3 + 1 + 1 + R.S_SIGMOID
    case = R.real_case('f32', seed=5, **CONFIGS['B'])
    ref, bound = R.pool_statement(case['feat'], case['rois'], *R.args_of(case))
    assert bool((bound >= 0).all()) and float(bound.max()) < 64 * R.U * float(ref.abs().max()) * 4


# ------------------------------------------------------------------------------------------------ module surface
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dpool_modules.json')


def _golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('i', range(7))
def test_modules_construct_with_the_reference_parameters(i):
    g = _golden_cases()[i]
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in g['kwargs'].items()}
    m = getattr(ops, g['cls'])(**kw)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == g['keys']
    assert [k for k, v in sd.items() if not bool(v.any())] == g['zero']
    for a, v in g['attrs'].items():
        mine = getattr(m, a)
        assert (list(mine) if isinstance(mine, tuple) else mine) == v, a
    # a reference state dict loads strictly
    m.load_state_dict({k: torch.randn(v.shape) for k, v in sd.items()}, strict=True)
    if g['keys']:
        assert isinstance(m.offset_fc, torch.nn.Sequential) and isinstance(m.offset_fc[0], torch.nn.Linear)


def test_the_fixture_covers_the_three_classes():
    assert len(_golden_cases()) == 7
    assert {g['cls'] for g in _golden_cases()} == {'DeformRoIPooling', 'DeformRoIPoolingPack', 'ModulatedDeformRoIPoolingPack'}


ROI_LAYER = dict(type='DeformRoIPoolingPack', out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1)


def _build(builtin, roi_layer):
    cfg = builtin()
    cfg.model.bbox_roi_extractor['roi_layer'] = dict(roi_layer)
    return registry.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('builtin', [selsa_config, hvr_config])
def test_a_config_with_a_deformable_roi_layer_builds_and_loads_strictly(builtin):
    model = _build(builtin, ROI_LAYER)
    plain = builtin()
    base = registry.build_detector(plain.model, train_cfg=plain.get('train_cfg'), test_cfg=plain.get('test_cfg'))
    layer = model.bbox_roi_extractor.roi_layers[0]
    assert isinstance(layer, ops.DeformRoIPoolingPack) and layer.spatial_scale == 1 / 16 and layer.out_size == (7, 7)
    new = set(model.state_dict()) - set(base.state_dict())
    assert new == {'bbox_roi_extractor.roi_layers.0.offset_fc.%d.%s' % (i, t) for i in (0, 2, 4) for t in ('weight', 'bias')}
    sd = model.state_dict()
    assert tuple(sd['bbox_roi_extractor.roi_layers.0.offset_fc.0.weight'].shape) == (1024, 12544)
    assert tuple(sd['bbox_roi_extractor.roi_layers.0.offset_fc.4.weight'].shape) == (98, 1024)
    ref_sd = {k: torch.randn(v.shape) if v.dtype.is_floating_point else v.clone() for k, v in sd.items()}
    model.load_state_dict(ref_sd, strict=True)
    with pytest.raises(RuntimeError):
        base.load_state_dict(ref_sd, strict=True)
    from hvrnet_amd.backbone import PackedMixin, set_compute_dtype
    assert isinstance(layer, PackedMixin)
    set_compute_dtype(model, torch.float16)
    assert layer.compute_dtype == torch.float16


def test_a_cpu_map_is_refused_and_there_is_no_backward():
    data, rois = torch.zeros((1, 8, 5, 5)), torch.tensor([[0, 0.0, 0.0, 30.0, 30.0]])
    with pytest.raises(NotImplementedError):
        ops.deform_roi_pooling(data, rois, data.new_empty(0), 1 / 16, 3, 8, True)
    with pytest.raises(NotImplementedError):
        ops.DeformRoIPooling(1 / 16, 3, 8, True)(data, rois, None)
    with pytest.raises(NotImplementedError):
        ops.DeformRoIPoolingPack(1 / 16, 3, 8, False, deform_fc_channels=16)(data, rois)
    with pytest.raises(NotImplementedError):
        ops.ModulatedDeformRoIPoolingPack(1 / 16, 3, 8, True)(data, rois)
    with pytest.raises(NotImplementedError, match='inference only'):
        ops.DeformRoIPoolingFunction.backward(None, torch.zeros(1))
    with pytest.raises(AssertionError):                                # deform_pool.py:150 / :230
        ops.DeformRoIPoolingPack(1 / 16, 3, 4, True)(data, rois)
    with pytest.raises(AssertionError):                                # deform_pool.py:28, :40
        ops.deform_roi_pooling(data, rois, data.new_empty(0), 1 / 16, (3, 4), 8, True)
    with pytest.raises(AssertionError):
        ops.deform_roi_pooling(data, rois, data.new_empty(0), 1 / 16, 3, 8, True, 1, None, 4, 1.5)


def test_training_entry_points_refuse_a_deformable_roi_layer_by_name():
    selsa = _build(selsa_config, ROI_LAYER)
    with pytest.raises(NotImplementedError, match='DeformRoIPoolingPack'):
        selsa.forward_train_sampled(None, None, None, None, None, None, None)
    with pytest.raises(NotImplementedError, match='DeformRoIPoolingPack'):
        selsa.forward_train(None, None, None, None)
    hvr = _build(hvr_config, dict(ROI_LAYER, type='ModulatedDeformRoIPoolingPack'))
    with pytest.raises(NotImplementedError, match='ModulatedDeformRoIPoolingPack'):
        hvr.forward_train(None, None, None, None)
    assert selsa._train_roi_layer.__doc__ and isinstance(_build(selsa_config, dict(type='RoIAlign', out_size=7, sample_num=2))._train_roi_layer(),
                                                         ops.RoIAlign)
