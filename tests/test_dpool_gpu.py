"""GPU tests of deformable RoI pooling: the kernel (hvr_deform_roi_pool_fwd) against the f64 statement of tests/dpool_refs.py in all
four compute modes, the exact families (equality with round-to-nearest of the statement), the refusals, the pooling packs against the
hand-made chain of public native calls, and an HVR window whose roi_layer is ModulatedDeformRoIPoolingPack: eager / graphed, the
cached per-frame path against the clip path, and its RoI features inside the statement's bracket."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dpool_refs as R  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': SPLIT, 'f32': torch.float32}
GUARD_ROWS = 8
SENTINEL = 7777

CONFIGS = {   # (tests/test_dpool_refs.py holds every listed mistake outside the bound on A, B and C)
    'A': dict(B=2, H=9, W=11, out_channels=64, K=40, P=7, spp=4, ps=7),
    'B': dict(B=2, H=9, W=11, out_channels=32, K=24, P=3, spp=2, ps=2, ncls=2),
    'C': dict(B=2, H=9, W=11, out_channels=16, group_size=3, K=24, P=3, spp=4, ps=3),
    'D': dict(B=2, H=9, W=11, out_channels=512, K=3, P=7, spp=4, ps=7, check=False, pick=(0, 5, 7)),   # one wide case: whole map, .5 corners, over the far border
    'E': dict(B=2, H=9, W=11, out_channels=64, K=40, P=7, spp=4, ps=7, ldt=100, ldm=52),
    'odd_spp': dict(B=2, H=9, W=11, out_channels=96, K=24, P=5, spp=3, ps=5),       # the any-sample_per_part instance; 12 / 24 lanes: no divisor of 256
}


def _pool(case, mode, with_trans=True, with_mask=True):
    """Runs the kernel on the case (true values on the CPU) into a sentinel-filled buffer with guard rows behind the output (split
    half has no `out=`: it is pooled in f32 and converted).  trans / mask_logit go over as column slices of their wide buffers.
    -> (stored values f64 on the CPU [K, P, P, Cout], guard rows untouched)"""
    fd = R.to_device_operand(case['feat'], mode, DEV)
    rois = case['rois'].to(DEV)
    K, P, Cout = rois.shape[0], case['P'], case['out_channels']
    trans = case['trans_buf'].to(DEV)[:, :case['trans'].shape[1]] if with_trans and case['trans'] is not None else None
    mask = case['mask_buf'].to(DEV)[:, :P * P] if with_mask and case['mask_logit'] is not None else None
    if trans is not None and 'trans_buf' in case and case['trans_buf'].shape[1] != case['trans'].shape[1]:
        assert trans.stride(0) == case['trans_buf'].shape[1] and not trans.is_contiguous()
    args = (case['P'], Cout, case['group_size'], case['part_size'], case['sample_per_part'], case['spatial_scale'], case['trans_std'])
    if mode == 'f16x2':
        out = native.deform_roi_pool(fd, rois, trans, mask, *args)
        torch.cuda.synchronize()
        return F.values(out).cpu(), True
    n = K * P * P * Cout
    buf = torch.full((n + GUARD_ROWS * P * P * Cout,), SENTINEL, dtype=DTYPES[mode], device=DEV)
    out = native.deform_roi_pool(fd, rois, trans, mask, *args, out=buf[:n].view(K, P, P, Cout))
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()), 'an output element was not written'
    return F.values(out).cpu(), bool((buf[n:] == SENTINEL).all())


def _hold(got, ref, bound, mode, what):
    lo, hi = R.stored_bracket(ref, bound, mode)
    ratio, bad, worst = F.compare(got, lo, hi, ref)
    print('%s %s: worst |got - ref| / bracket = %.3f, %d of %d outside' % (what, mode, ratio, bad, ref.numel()))
    assert bad == 0, (what, mode, ratio, bad, worst)


# ------------------------------------------------------------------------------------------------ kernel vs statement
@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_kernel_lies_in_the_bracket_of_the_statement(mode, name):
    """Every configuration with offsets and mask, with offsets alone and (pass 1) with neither.  The cases carry empty, partial and
    full bins, .5 corners of both signs, degenerate, off-map and whole-map RoIs (asserted by the generator)."""
    case = R.real_case(mode, seed=17, **CONFIGS[name])
    for with_trans, with_mask in ((True, True), (True, False), (False, False), (False, True)):
        ref, bound = R.pool_statement(case['feat'], case['rois'], *R.args_of(case, with_trans, with_mask))
        got, guard = _pool(case, mode, with_trans, with_mask)
        assert guard, 'guard rows behind the output were written'
        assert float(ref.abs().max()) > 0.3
        _hold(got, ref, bound, mode, '%s trans %d mask %d' % (name, with_trans, with_mask))


def test_offsets_may_come_as_a_4d_tensor_and_the_batch_index_selects_the_frame():
    case = R.real_case('f32', seed=19, **CONFIGS['B'])
    fd, rois = R.to_device_operand(case['feat'], 'f32', DEV), case['rois'].to(DEV)
    a = native.deform_roi_pool(fd, rois, case['trans'].to(DEV), None, 3, 32, 1, 2, 2, 1 / 16, 0.1)
    b = native.deform_roi_pool(fd, rois, case['trans'].to(DEV).view(-1, 4, 2, 2).contiguous(), None, (3, 3), 32, 1, 2, 2, 1 / 16, 0.1)
    assert torch.equal(a, b)
    swapped = rois.clone()
    swapped[:, 0] = 1 - swapped[:, 0]
    c = native.deform_roi_pool(fd.flip(0).contiguous(), swapped, case['trans'].to(DEV), None, 3, 32, 1, 2, 2, 1 / 16, 0.1)
    assert torch.equal(a, c) and float(a.abs().max()) > 0.3
    assert tuple(native.deform_roi_pool(fd, rois[:0], None, None, 3, 32, 1, 2, 2, 1 / 16, 0.1).shape) == (0, 3, 3, 32)


# ------------------------------------------------------------------------------------------------ exact families
# ('lo_act': wide values with a non-zero lo half exist in the split-half format only)
@pytest.mark.parametrize('mode,family', [(m, f) for m in F.MODES for f in R.EXACT_FAMILIES if f != 'lo_act'] + [('f16x2', 'lo_act')])
def test_exact_families_equal_the_rounded_statement(mode, family):
    for (P, spp) in ((4, 2), (2, 4)):
        case = R.exact_case(mode, 21, family, P=P, spp=spp)
        case['trans_buf'], case['mask_buf'] = case['trans'], case['mask_logit']
        ref, _ = R.pool_statement(case['feat'], case['rois'], *R.args_of(case))
        want = F.round_stored(ref.float().double(), mode)
        got, guard = _pool(case, mode)
        assert guard
        nbad = int((got != want).sum())
        assert nbad == 0, (family, mode, P, spp, nbad)
        if family == 'outside':
            assert not bool(got.any())
        if family == 'zero':                                         # zero offsets given == no offsets
            none, _ = _pool(case, mode, with_trans=False)
            assert torch.equal(none, got)
        if family == 'lo_act':
            assert bool((F.split_parts(want, F.ACT_SCALE)[1] != 0).any())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_with_a_message():
    x = torch.zeros((1, 5, 5, 64), dtype=torch.bfloat16, device=DEV)
    rois = torch.tensor([[0, 0.0, 0.0, 40.0, 40.0]], device=DEV)
    with pytest.raises(native.HvrError, match=r'out_channels \* group_size\^2'):
        native.deform_roi_pool(x, rois, None, None, 3, 32, 1, 3, 4, 1 / 16, 0.0)
    with pytest.raises(native.HvrError, match=r'out_channels \* group_size\^2'):
        native.deform_roi_pool(x, rois, None, None, 3, 64, 2, 3, 4, 1 / 16, 0.0)
    with pytest.raises(native.HvrError, match='not square'):
        native.deform_roi_pool(x, rois, None, None, (3, 4), 64, 1, 3, 4, 1 / 16, 0.0)
    with pytest.raises(native.HvrError, match='offset classes'):
        native.deform_roi_pool(x[..., :36].contiguous(), rois, torch.zeros((1, 5 * 2 * 9), device=DEV), None, 3, 36, 1, 3, 4, 1 / 16, 0.1)
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(native.HvrError, match='trans_std'):
            native.deform_roi_pool(x, rois, None, None, 3, 64, 1, 3, 4, 1 / 16, bad)
    with pytest.raises(native.HvrError, match='part_size'):
        native.deform_roi_pool(x, rois, torch.zeros((1, 17), device=DEV), None, 3, 64, 1, 3, 4, 1 / 16, 0.1)
    with pytest.raises(native.HvrError, match='mask logits'):
        native.deform_roi_pool(x, rois, None, torch.zeros((1, 10), device=DEV), 3, 64, 1, 3, 4, 1 / 16, 0.1)
    lib = native.lib()
    rc = lib.hvr_deform_roi_pool_fwd(native._ptr(x), native._ptr(rois), None, None, native._ptr(x), 1, 5, 5, 64, 1, 3, 3, 64, 1, 3, 1, 4, 1 / 16, 0.0, 0, 0,
                                     native.HVR_F16S, None)
    assert rc != 0 and b'split-half' in lib.hvr_last_error()
    assert lib.hvr_abi_version() == 7


# ------------------------------------------------------------------------------------------------ packs vs the hand-made chain
PACK_KW = dict(spatial_scale=1 / 16, out_size=7, out_channels=64, no_trans=False, group_size=1, trans_std=0.1, deform_fc_channels=128)


def _randomise(pack, seed):
    """Non-zero offset and mask weights: hidden layers N(0, 1 / fan_in), the last layers sized for offsets of a few units and logits ~ 1."""
    g = torch.Generator().manual_seed(seed)
    for name in ('offset_fc', 'mask_fc'):
        fcs = [m for m in getattr(pack, name, ()) if isinstance(m, torch.nn.Linear)]
        for i, fc in enumerate(fcs):
            std = (1.0 / fc.in_features) ** 0.5 * (3.0 if i == len(fcs) - 1 else 1.4)
            fc.weight.data = torch.randn(fc.weight.shape, generator=g) * std
            fc.bias.data = torch.randn(fc.bias.shape, generator=g) * 0.1
    return pack


def _hwc(w, C, P):
    return w.view(-1, C, P, P).permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _padded(w, b, dt):
    """The last layer of a chain as the pack must hold it: rows padded with zeros to a multiple of 4."""
    n = (w.shape[0] + 3) // 4 * 4
    wp, bp = torch.zeros((n, w.shape[1]), device=w.device), torch.zeros(n, device=w.device)
    wp[:w.shape[0]], bp[:w.shape[0]] = w, b
    return native.as_operand(wp, dt), bp


def _hand_chain(pack, fmap, rois):
    """The pack's forward as public native calls on operands packed here from the module's parameters: pass 1, the first layers as TWO
    GEMMs, the remaining layers, pass 2.  fmap: the physical NHWC map in the pack's compute dtype.  -> dict of the links."""
    dt = pack.compute_dtype
    P, C = pack.out_size[0], pack.out_channels
    pool = lambda f, t, m: native.deform_roi_pool(f, rois, t, m, P, C, pack.group_size, pack.part_size, pack.sample_per_part,
                                                  pack.spatial_scale, pack.trans_std)
    f = native.cast(fmap, torch.float32) if dt == SPLIT else fmap
    x1 = pool(f, None, None)
    rows = x1.view(rois.shape[0], -1)
    rows = native.cast(rows, dt) if dt == SPLIT else rows
    out = dict(x1=x1, rows=rows, fmap=f)
    logits = {}
    for name in ('offset_fc', 'mask_fc'):
        fcs = [m for m in getattr(pack, name, ()) if isinstance(m, torch.nn.Linear)]
        if not fcs:
            continue
        h = rows
        for i, fc in enumerate(fcs):
            last = i == len(fcs) - 1
            w = fc.weight.detach().float()
            w = _hwc(w, C, P) if i == 0 else w
            b = fc.bias.detach().float().contiguous()
            wq, b = _padded(w, b, dt) if last else (native.as_operand(w, dt), b)
            h = native.gemm(h, wq, b, relu=not last, out_f32=last)
            if i == 0 and not last:
                out[name + '_h0'] = h
        assert h.dtype == torch.float32 and h.shape[1] % 4 == 0
        logits[name] = h
    trans = logits['offset_fc'][:, :2 * P * P]
    mask = logits['mask_fc'][:, :P * P] if 'mask_fc' in logits else None
    y = pool(f, trans, mask)
    out.update(trans=trans, mask=mask, y=native.cast(y, dt) if dt == SPLIT else y, y_f32=y)
    return out


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('cls', ['DeformRoIPoolingPack', 'ModulatedDeformRoIPoolingPack'])
def test_packs_equal_the_hand_made_chain_bit_for_bit(mode, cls):
    case = R.real_case(mode, seed=23, **CONFIGS['A'])
    pack = _randomise(getattr(ops, cls)(**PACK_KW), 24).to(DEV).eval()
    backbone.set_compute_dtype(pack, DTYPES[mode])
    fmap = R.to_device_operand(case['feat'], mode, DEV)
    rois = case['rois'].to(DEV)
    with torch.no_grad():
        y = pack(backbone.as_logical(fmap), rois)
        hand = _hand_chain(pack, fmap, rois)
        p = pack.packed(fmap.device)
    assert tuple(y.shape) == (40, 64, 7, 7) and ops._channels_last(y)              # the logical view of [K, P, P, C]: BBoxHead's fc1_hwc route
    assert torch.equal(y.permute(0, 2, 3, 1), hand['y'])
    assert tuple(hand['trans'].shape) == (40, 98) and hand['trans'].stride(0) == 100
    assert float(hand['trans'].abs().max()) > 1.0 and float(F.values(hand['y']).abs().max()) > 0.3
    if cls == 'ModulatedDeformRoIPoolingPack':
        # the fused first layer (ONE GEMM of 2 x 128 outputs) equals the two separate GEMMs bit for bit
        assert hand['mask'].stride(0) == 52 and float(hand['mask'].abs().max()) > 0.5
        h = native.gemm(hand['rows'], p['fused0'][0], p['fused0'][1], relu=True)
        assert tuple(h.shape) == (40, 256) and p['fused_split'] == 128
        assert torch.equal(h[:, :128], hand['offset_fc_h0']) and torch.equal(h[:, 128:], hand['mask_fc_h0'])
        assert float(F.values(h).abs().max()) > 0.1
    else:
        assert 'fused0' not in p and hand['mask'] is None
    # pass 2 against the statement on the device's own offsets and logits
    ref, bound = R.pool_statement(F.values(fmap).cpu(), case['rois'], hand['trans'].cpu(), None if hand['mask'] is None else hand['mask'].cpu(),
                                  7, 64, 1, 7, 4, 1 / 16, 0.1)
    _hold(F.values(hand['y']).cpu(), ref, bound, mode, cls)
    # an NCHW-contiguous map is converted once and gives the same result
    if mode != 'f16x2':
        with torch.no_grad():
            y2 = pack(backbone.as_logical(fmap).contiguous(), rois)
        assert torch.equal(y2, y)


@pytest.mark.parametrize('mode', F.MODES)
def test_freshly_initialised_packs_give_pass_one_and_half_of_it(mode):
    """The last offset / mask layers start at zero: v1 is pass 1; v2 is sigmoid(0) = exactly half of it before the store -- stated
    through the statement's bracket with zero offsets and zero logits.  no_trans packs are pass 1 alone."""
    case = R.real_case(mode, seed=25, **CONFIGS['A'])
    fmap = R.to_device_operand(case['feat'], mode, DEV)
    rois = case['rois'].to(DEV)
    zt, zm = torch.zeros((40, 98)), torch.zeros((40, 49))
    one, bound1 = R.pool_statement(case['feat'], case['rois'], zt, None, 7, 64, 1, 7, 4, 1 / 16, 0.1)
    half, bound2 = R.pool_statement(case['feat'], case['rois'], zt, zm, 7, 64, 1, 7, 4, 1 / 16, 0.1)
    assert torch.equal(half, one * 0.5)
    for cls, ref, bound in (('DeformRoIPoolingPack', one, bound1), ('ModulatedDeformRoIPoolingPack', half, bound2)):
        pack = getattr(ops, cls)(**PACK_KW).to(DEV).eval()
        for fc in (pack.offset_fc[0], pack.offset_fc[2]):
            assert float(fc.weight.detach().abs().max()) > 0
        backbone.set_compute_dtype(pack, DTYPES[mode])
        with torch.no_grad():
            y = pack(backbone.as_logical(fmap), rois)
        _hold(F.values(y.permute(0, 2, 3, 1)).cpu(), ref, bound, mode, cls + ' fresh')
        plain = getattr(ops, cls)(**dict(PACK_KW, no_trans=True)).to(DEV).eval()
        backbone.set_compute_dtype(plain, DTYPES[mode])
        with torch.no_grad():
            y0 = plain(backbone.as_logical(fmap), rois)
            x1 = native.deform_roi_pool(fmap, rois, None, None, 7, 64, 1, 7, 4, 1 / 16, 0.1)
        assert torch.equal(y0.permute(0, 2, 3, 1), x1)
        if cls == 'DeformRoIPoolingPack':
            assert torch.equal(y, y0)                                               # zero offsets: pass 2 IS pass 1
    # the plain module and the Function: offsets in the reference's [K, 2, P, P] shape
    with torch.no_grad():
        t = (torch.randn((40, 2, 7, 7), generator=torch.Generator().manual_seed(26)) * 3).to(DEV)
        m = ops.DeformRoIPooling(1 / 16, 7, 64, False, trans_std=0.1)
        y = m(backbone.as_logical(fmap), rois, t)
        assert torch.equal(y.permute(0, 2, 3, 1), native.deform_roi_pool(fmap, rois, t, None, 7, 64, 1, 7, 4, 1 / 16, 0.1))


# ------------------------------------------------------------------------------------------------ a window with deformable pooling
HW, PAD = (150, 250), (160, 256)          # the reduced window of tests/test_dcn_gpu.py
T, NPROP = 3, 24
ROI_LAYER = dict(type='ModulatedDeformRoIPoolingPack', out_size=7, out_channels=256, no_trans=False, group_size=1, trans_std=0.1,
                 deform_fc_channels=256)
_models = {}


def _window_model(dtype):
    """HNMBRCNN at depth 50 with synthetic weights and the modulated pooling pack as its roi_layer (non-zero offset / mask weights)."""
    if dtype not in _models:
        cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
        cfg.model.backbone['depth'] = 50
        cfg.model.shared_head['depth'] = 50
        cfg.model.bbox_roi_extractor['roi_layer'] = dict(ROI_LAYER)
        sd = S.synth_state_dict('hvr', depth=50)
        kw = {k: v for k, v in ROI_LAYER.items() if k != 'type'}
        pack = _randomise(ops.ModulatedDeformRoIPoolingPack(spatial_scale=1 / 16, **kw), 91)
        for k, v in pack.state_dict().items():
            sd['bbox_roi_extractor.roi_layers.0.' + k] = v
        _models[dtype] = hvrnet_amd.build_model(cfg, sd, dtype, DEV)
    return _models[dtype]


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _clip(seed):
    return torch.cat([S.synth_frame(seed + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)


def test_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert isinstance(model.bbox_roi_extractor.roi_layers[0], ops.ModulatedDeformRoIPoolingPack)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [_clip(10 * c) for c in range(2)]
    first = [_eager(model, clip, metas) for clip in clips]
    again = [_eager(model, clip, metas) for clip in clips]
    g = GraphedClip(model, clips[0], metas, rescale=True)
    n_det = 0
    for rep in range(2):
        for clip, want, want2 in zip(clips, first, again):
            got = g.run(clip).result()
            assert len(got) == len(want) == 2
            assert all(_same(a, b) for a, b in zip(want, want2)), 'two eager calls differ'
            assert all(_same(a, b) for a, b in zip(got, want)), 'graph replay differs from the eager window'
            n_det += sum(len(r) for r in got[-1])
    assert n_det > 0


def test_cached_frame_path_gives_the_clip_paths_fc1_rows():
    model = _window_model(torch.bfloat16)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = _clip(40)
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        w = model.window_tensors(c4, metas, speculate=True)
        f1 = model.bbox_head.fc1_rows(w['roi_feats'])
        assert tuple(f1.shape) == (T * NPROP, 1024) and ops._channels_last(w['roi_feats'])
        for i in range(T):
            e = model.frame_tensors(c4[i:i + 1], metas[i])
            assert torch.equal(e['f1'], f1[i * NPROP:(i + 1) * NPROP]), i
    assert float(f1.float().abs().max()) > 0


def test_window_roi_feats_lie_in_the_bracket_of_the_statement_in_f32():
    """f32 mode: the window's roi_feats against the statement on the window's own c5 map and RoIs, with the offsets and logits its
    own FC chain produced (recomputed here as public native calls)."""
    model = _window_model(torch.float32)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = _clip(70)
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        w = model.window_tensors(c4, metas)
        pack = model.bbox_roi_extractor.roi_layers[0]
        fmap = w['c5'].permute(0, 2, 3, 1)
        assert fmap.is_contiguous() and fmap.dtype == torch.float32
        rois = w['rois'].contiguous()
        hand = _hand_chain(pack, fmap, rois)
    got = w['roi_feats'].permute(0, 2, 3, 1)
    assert torch.equal(got, hand['y'])
    ref, bound = R.pool_statement(fmap.cpu(), rois.cpu(), hand['trans'].cpu(), hand['mask'].cpu(), 7, 256, 1, 7, 4, 1 / 16, 0.1)
    assert float(hand['trans'].abs().max()) > 0.5 and float(ref.abs().max()) > 0
    _hold(got.double().cpu(), ref, bound, 'f32', 'window roi_feats')
