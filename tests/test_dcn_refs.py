"""CPU checks of the deformable-conv statement (tests/dcn_refs.py) and of the dcn module surface (-m "not gpu"):
the statement against torch's grid_sample in f64, an independent f32 evaluation of the rule inside the bound, every listed mistake
outside it (or unequal on the exact families), and the constructors / checkpoint contract of the dcn modules."""
import pytest
import torch
import torch.nn.functional as TF

from hvrnet_amd import backbone, registry
from hvrnet_amd.config import hvr_config, selsa_config
from tests import dcn_refs as D
from tests import forward_kernel_refs as F

MODES = F.MODES


def test_statement_equals_grid_sample_in_f64():
    """A 1x1 kernel at stride 1 without padding samples pixel + offset: the statement must equal bilinear grid_sample with zero
    padding and align_corners=True (positions in pixel units) -- also at -1, H - 1, H - 0.5 and H exactly."""
    B, H, W, C = 2, 9, 11, 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, H, W, C), generator=g, dtype=torch.float64)
    ty = torch.cat([torch.tensor([-1.0, H - 1.0, H - 0.5, float(H), -1.5, -0.5, 0.0]), torch.rand(H * W - 7, generator=g) * (H + 2) - 1.5])
    tx = torch.cat([torch.tensor([0.5, W - 1.0, W - 0.5, 2.0, 3.0, -1.0, float(W)]), torch.rand(H * W - 7, generator=g) * (W + 2) - 1.5])
    oy = torch.arange(H)[:, None].expand(H, W).float()
    ox = torch.arange(W)[None, :].expand(H, W).float()
    om = torch.zeros((B, H, W, 2))
    om[..., 0] = ty.view(H, W) - oy
    om[..., 1] = tx.view(H, W) - ox
    ref, _ = D.sampler_statement(x, om, 1, 1, 1, 0, 1, 1, False)
    py = (oy + om[0, ..., 0]).double()        # the positions the statement used (f32 adds)
    px = (ox + om[0, ..., 1]).double()
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1)[None].expand(B, H, W, 2)
    gs = TF.grid_sample(x.permute(0, 3, 1, 2), grid, mode='bilinear', padding_mode='zeros', align_corners=True).permute(0, 2, 3, 1)
    diff = float((gs.reshape(B * H * W, C) - ref).abs().max())
    print('statement vs grid_sample: max |diff| = %.3g on %d positions' % (diff, H * W))
    assert diff <= 1e-13
    # the drop test and the open border: exact zeros where the rule says so
    r = ref.view(B, H * W, C)
    assert bool((r[:, 0] == 0).all()) and bool((r[:, 3] == 0).all()) and bool((r[:, 4] == 0).all())
    assert bool((r[:, 1] == x[:, H - 1, W - 1]).all())


def _f32_rule(x, om, KH, KW, stride, pad, dil, dg, modulated, order):
    """An f32 evaluation of the rule, every operation rounded on its own, the four products joined sequentially (order 0) or
    pairwise (order 1).  x f32 true values."""
    x = x.float()
    B, H, W, C = x.shape
    OH, OW = D.out_hw(H, W, KH, KW, stride, pad, dil)
    KK, cpg = KH * KW, C // dg
    out = torch.zeros((B, OH, OW, KK, C), dtype=torch.float32)
    bi = torch.arange(B)[:, None, None].expand(B, OH, OW)
    for kh in range(KH):
        for kw in range(KW):
            k = kh * KW + kw
            for g in range(dg):
                h = (torch.arange(OH)[None, :, None] * stride - pad + kh * dil).float() + om[..., g * 2 * KK + 2 * k]
                w = (torch.arange(OW)[None, None, :] * stride - pad + kw * dil).float() + om[..., g * 2 * KK + 2 * k + 1]
                inside = (h > -1) & (w > -1) & (h < H) & (w < W)
                hl, wl = torch.floor(h), torch.floor(w)
                lh, lw = h - hl, w - wl
                hh, hw = 1 - lh, 1 - lw
                t = []
                for dy, dx, wgt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
                    yi, xi = hl + dy, wl + dx
                    ok = (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1) & inside
                    v = x[bi, yi.clamp(0, H - 1).long(), xi.clamp(0, W - 1).long(), g * cpg:(g + 1) * cpg] * ok[..., None]
                    t.append(wgt[..., None] * v)
                val = ((t[0] + t[1]) + t[2]) + t[3] if order == 0 else (t[0] + t[1]) + (t[2] + t[3])
                if modulated:
                    val = val * (1 / (1 + torch.exp(-om[..., 2 * dg * KK + g * KK + k])))[..., None]
                out[:, :, :, k, g * cpg:(g + 1) * cpg] = val
    return out.view(B * OH * OW, KK * C)


CASES = [  # B, H, W, C, stride, pad, dil, dg, modulated
    (2, 5, 7, 64, 1, 1, 1, 2, True),
    (1, 6, 5, 64, 1, 2, 2, 4, False),
    (2, 7, 6, 32, 2, 1, 1, 1, True),
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('order', [0, 1])
def test_f32_evaluation_lies_inside_the_bound(case, order):
    B, H, W, C, s, p, d, dg, mod = case
    for mode in MODES:
        x, om = D.real_inputs(B, H, W, C, 3, 3, s, p, d, dg, mod, mode, seed=11, ldo=3 * dg * 9 + 5)
        ref, bound = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
        got = _f32_rule(x, om, 3, 3, s, p, d, dg, mod, order).double()
        ratio, bad, _ = F.compare(got, ref - bound, ref + bound, ref)
        print('%s order %d: worst |f32 - ref| / bound = %.3f' % (mode, order, ratio))
        assert bad == 0 and float(ref.abs().max()) > 0.5
        if mode != 'f32':                               # the stored form of that f32 value lies in the bracket
            lo, hi = D.stored_bracket(ref, bound, mode)
            assert F.compare(F.round_stored(got, mode), lo, hi, ref)[1] == 0


def _config_for(mistake):
    # stride, pad, dil, dg, modulated: a configuration in which the mistake changes something
    if mistake == 'dil1':
        return 1, 2, 2, 2, True
    if mistake == 'stride1':
        return 2, 1, 1, 2, True
    return 1, 1, 1, 2, True


@pytest.mark.parametrize('mistake', [m for m in D.MISTAKES if m != 'rows_past_M'])
@pytest.mark.parametrize('mode', MODES)
def test_every_mistake_falls_outside_the_bound(mistake, mode):
    s, p, d, dg, mod = _config_for(mistake)
    x, om = D.real_inputs(2, 5, 7, 64, 3, 3, s, p, d, dg, mod, mode, seed=3)
    ref, bound = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
    lo, hi = D.stored_bracket(ref, bound, mode)
    wrong, _ = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod, mistake=mistake)
    stored = wrong if mode == 'f32' else F.round_stored(wrong.float().double(), mode)
    ratio, bad, _ = F.compare(stored, lo, hi, ref)
    right = ref if mode == 'f32' else F.round_stored(ref.float().double(), mode)
    assert F.compare(right, lo, hi, ref)[1] == 0            # the statement itself passes ...
    assert bad > 0 and ratio > 10.0, (mistake, mode, bad, ratio)   # ... the mistake does not, by far


@pytest.mark.parametrize('mistake', [m for m in D.MISTAKES if m != 'rows_past_M'])
def test_every_mistake_is_unequal_on_an_exact_family(mistake):
    s, p, d, dg, mod = _config_for(mistake)
    fam = 'border' if mistake in ('border_closed', 'corner_clamped') else 'eighths'
    x, om = D.exact_inputs(2, 5, 7, 64, 3, 3, s, p, d, dg, mod, 'bf16', seed=4, family=fam)
    ref, _ = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod)
    wrong, _ = D.sampler_statement(x, om, 3, 3, s, p, d, dg, mod, mistake=mistake)
    assert not torch.equal(F.round_stored(ref, 'bf16'), F.round_stored(wrong, 'bf16'))


@pytest.mark.parametrize('mode', MODES)
def test_rows_past_M_breaks_the_guard(mode):
    x, om = D.real_inputs(2, 5, 7, 64, 3, 3, 1, 1, 1, 1, False, mode, seed=3)
    ref, _ = D.sampler_statement(x, om, 3, 3, 1, 1, 1, 1, False)
    M = ref.shape[0]
    assert M % 64 != 0
    assert F.guard_intact(F.emulate_store(ref, mode), M)
    assert not F.guard_intact(F.emulate_store(ref, mode, mistake='rows_past_M'), M)


@pytest.mark.parametrize('family', ['zero', 'integer', 'eighths', 'border', 'lo_act'])
def test_exact_families_are_exact_in_f32(family):
    """On the exact families the independent f32 evaluation, in either association, EQUALS the statement."""
    mode = 'f16x2' if family == 'lo_act' else 'bf16'
    for mod in (False, True):
        x, om = D.exact_inputs(2, 5, 7, 64, 3, 3, 1, 1, 1, 2, mod, mode, seed=8, family=family)
        ref, _ = D.sampler_statement(x, om, 3, 3, 1, 1, 1, 2, mod)
        ref = ref.float().double()      # RN to f32: sigmoid(32) and sigmoid(-128) are 1 and 0 to f32 precision, 1 - 1e-14 and 3e-56 in f64
        for order in (0, 1):
            assert torch.equal(_f32_rule(x, om, 3, 3, 1, 1, 1, 2, mod, order).double(), ref)
        if family == 'zero' and not mod:
            cols, _, _ = F._patches(x, 3, 3, 1, 1, 1)
            assert torch.equal(cols, ref)
        if family == 'lo_act':
            hi, lo = F.split_parts(ref, F.ACT_SCALE)
            assert bool((lo != 0).any()) and torch.equal(hi + lo, ref)
        if family == 'border':
            assert bool((ref != 0).any())


# ------------------------------------------------------------------------------------------------ module surface
DCNS = [dict(modulated=False, deformable_groups=1, fallback_on_stride=False), dict(modulated=True, deformable_groups=2, fallback_on_stride=False)]


def _dcn_cfg(builtin, dcn):
    cfg = builtin()
    cfg.model.backbone['dcn'] = dcn
    cfg.model.backbone['stage_with_dcn'] = (False, False, True)
    cfg.model.shared_head['dcn'] = dcn
    return cfg


@pytest.mark.parametrize('builtin', [selsa_config, hvr_config])
@pytest.mark.parametrize('dcn', DCNS)
def test_reference_configs_with_dcn_build_and_load_strictly(builtin, dcn):
    cfg = _dcn_cfg(builtin, dcn)
    model = registry.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    plain = builtin()
    base = registry.build_detector(plain.model, train_cfg=plain.get('train_cfg'), test_cfg=plain.get('test_cfg'))
    n_off = dcn['deformable_groups'] * (27 if dcn['modulated'] else 18)
    new = set(model.state_dict()) - set(base.state_dict())
    blocks = ['backbone.layer3.%d' % i for i in range(23)] + ['shared_head.layer4.%d' % i for i in range(3)]
    assert new == {'%s.conv2_offset.%s' % (b, t) for b in blocks for t in ('weight', 'bias')}
    sd = model.state_dict()
    for b, planes in [(blocks[0], 256), (blocks[-1], 512)]:
        assert tuple(sd[b + '.conv2_offset.weight'].shape) == (n_off, planes, 3, 3) and tuple(sd[b + '.conv2_offset.bias'].shape) == (n_off,)
        assert tuple(sd[b + '.conv2.weight'].shape) == (planes, planes, 3, 3) and (b + '.conv2.bias') not in sd
    # a reference state dict with these keys loads strictly; without them it does not
    ref_sd = {k: torch.randn(v.shape) if v.dtype.is_floating_point else v.clone() for k, v in sd.items()}
    model.load_state_dict(ref_sd, strict=True)
    with pytest.raises(RuntimeError):
        base.load_state_dict(ref_sd, strict=True)
    # layer 4 of the shared head: stride 1, dilation 2 -> the offset conv has the geometry of conv2
    oc = model.shared_head.layer4[0].conv2_offset
    assert oc.stride == (1, 1) and oc.padding == (2, 2) and oc.dilation == (2, 2) and oc.bias is not None
    assert not any(b.with_dcn for b in model.backbone.layer2)


def test_resnet_dcn_arguments():
    dcn = dict(modulated=True, deformable_groups=1, fallback_on_stride=True)
    net = backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='pytorch', dcn=dcn,
                          stage_with_dcn=(False, True, True))
    # fallback_on_stride: the stride-2 conv2 of a pytorch-style stage's first block stays a plain conv (resnet.py:150-152)
    assert not net.layer2[0].with_dcn and not hasattr(net.layer2[0], 'conv2_offset')
    assert net.layer2[1].with_dcn and net.layer2[1].with_modulated_dcn and net.layer2[1].conv2_offset.out_channels == 27
    assert not any(b.with_dcn for b in net.layer1)
    with pytest.raises(AssertionError):
        backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), dcn=dcn,
                        stage_with_dcn=(False, False, False, True))
    for bad in (dict(gcb=dict()), dict(gen_attention=dict()), dict(conv_cfg=dict(type='ConvWS'))):
        with pytest.raises(NotImplementedError):
            backbone.ResNet(depth=50, **bad)
    # a stage that ends in a dcn block is never compacted
    caffe = backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe',
                            dcn=dict(modulated=False, deformable_groups=1, fallback_on_stride=False), stage_with_dcn=(True, False, False))
    plain = backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
    assert plain._ends_compact(0) and not caffe._ends_compact(0)


def test_init_weights_zeroes_the_offset_conv_and_training_is_refused():
    dcn = dict(modulated=True, deformable_groups=2, fallback_on_stride=False)
    net = backbone.ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', dcn=dcn,
                          stage_with_dcn=(False, False, True))
    for b in net.layer3:
        torch.nn.init.normal_(b.conv2_offset.weight)
        torch.nn.init.normal_(b.conv2_offset.bias)
    net.init_weights()
    for b in net.layer3:
        assert float(b.conv2_offset.weight.abs().max()) == 0.0 and float(b.conv2_offset.bias.abs().max()) == 0.0
        assert float(b.conv2.weight.abs().max()) > 0.0
    with pytest.raises(NotImplementedError):
        net.layer3[0].forward_train_nhwc(torch.zeros((1, 4, 4, 512)))
    head = backbone.ResLayer(depth=50, stage=3, stride=1, dilation=2, style='caffe', dcn=dcn)
    assert all(b.with_dcn for b in head.layer4)
    with pytest.raises(NotImplementedError):
        head.forward_train_nhwc(torch.zeros((1, 4, 4, 1024)))
