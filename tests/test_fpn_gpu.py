"""GPU tests of the multi-level feature path: hvr_fpn_merge bit for bit against its rule (tests/fpn_refs.merge_rule), native.roi_align_levels
against the level rule, against native.roi_align_fwd per level (bit for bit) and against the per-level f64 statement, the FPN module in
the four compute modes against the hand-made chain of native calls and, in f32, against the reference's f64 outputs, SingleRoIExtractor
on the golden maps, and a ResNet-50 + FPN + extractor detector with the neck and the extraction captured in a hipGraph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import native  # noqa: E402
from hvrnet_amd.backbone import as_nhwc, set_compute_dtype  # noqa: E402
from hvrnet_amd.detectors import TwoStageDetector  # noqa: E402
from hvrnet_amd.necks import FPN, kstep_pad  # noqa: E402
from hvrnet_amd.roi_extractor import SingleRoIExtractor  # noqa: E402
from tests import fpn_refs as R  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
NHWC = native.LAYOUT_NHWC
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
# one rounding to the storage format: the unit roundoff 2^-p of its p significant bits (bf16 8, half 11), relative to the value, and for
# half half the spacing of its subnormals (2^-24), absolute
STORE_U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
STORE_ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 0.0}
SENTINEL = 7777.0
GUARD = 4096       # guard elements behind every output


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the merge kernel
def _laterals(L, B, base, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((B, base[0] >> l, base[1] >> l, C), generator=g) * 3).to(dtype) for l in range(L)]


def _guarded_like(ts):
    bufs = [torch.full((t.numel() + GUARD,), SENTINEL, dtype=t.dtype, device=DEV) for t in ts]
    return bufs, [b[:t.numel()].view(t.shape) for b, t in zip(bufs, ts)]


MERGE_CASES = [(m, 4, 1, (24, 40), 64) for m in ('bf16', 'f16', 'f32')]
MERGE_CASES += [('bf16', 2, 1, (24, 40), 64), ('f32', 1, 1, (24, 40), 64), ('f16', 4, 2, (24, 40), 64), ('bf16', 4, 1, (8, 8), 64),
                ('f32', 2, 1, (2, 2), 64), ('bf16', 4, 1, (24, 40), 256), ('f32', 4, 2, (24, 40), 12), ('f16', 3, 1, (8, 8), 256)]


@pytest.mark.parametrize('mode,L,B,base,C', MERGE_CASES)
def test_merge_equals_the_rule_bit_for_bit(mode, L, B, base, C):
    """The f32 sum in the stated order, rounded once, by torch on the CPU; inputs unchanged; guard elements intact; two runs and a
    captured graph give equal bits."""
    dtype = DTYPES[mode]
    host = _laterals(L, B, base, C, dtype, 1000 + L * 7 + C)
    want = R.merge_rule(host)
    lats = [t.to(DEV) for t in host]
    bufs, outs = _guarded_like(lats[:-1])
    got = native.fpn_merge(lats, out=outs)
    torch.cuda.synchronize()
    assert len(got) == L and got[-1] is lats[-1]
    for l in range(L - 1):
        nbad = int((bits(got[l].cpu()) != bits(want[l])).sum())
        print('fpn_merge %s L=%d level %d %s: %d of %d elements differ' % (mode, L, l, tuple(want[l].shape), nbad, want[l].numel()))
        assert nbad == 0
        assert bool((bufs[l][lats[l].numel():] == SENTINEL).all()), 'guard elements behind out[%d] were written' % l
    for a, b in zip(lats, host):
        assert same_bits(a.cpu(), b)
    again = native.fpn_merge(lats)
    if L == 1:          # nothing is launched: there is nothing to capture
        assert again[0] is lats[0]
        return
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap = native.fpn_merge(lats)
    torch.cuda.current_stream().wait_stream(side)
    for t in cap[:-1]:
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    for l in range(L - 1):
        assert same_bits(again[l], got[l]) and same_bits(cap[l], got[l])


def test_merge_refusals_write_nothing():
    lats = [t.to(DEV) for t in _laterals(3, 1, (8, 8), 64, torch.bfloat16, 5)]
    bufs, outs = _guarded_like(lats[:-1])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((b == SENTINEL).all()) for b in bufs)
    bad = [lats[0], lats[1][:, :3].contiguous(), lats[2]]
    with pytest.raises(native.HvrError, match='size mismatch'):
        native.fpn_merge(bad, out=[outs[0], torch.empty_like(bad[1])])
    with pytest.raises(native.HvrError, match='no instance'):       # bf16 needs C % 8 == 0
        native.fpn_merge([t[..., :12].contiguous() for t in lats])
    with pytest.raises(native.HvrError, match='aliases'):
        native.fpn_merge(lats, out=[lats[0], outs[1]])
    with pytest.raises(native.HvrError, match='aliases'):       # out[1] inside out[0]'s bytes
        native.fpn_merge(lats, out=[outs[0], bufs[0][:lats[1].numel()].view(lats[1].shape)])
    with pytest.raises(native.HvrError, match='split-half'):
        native.fpn_merge([native.cast(t.float(), SPLIT) for t in lats])
    assert untouched()
    assert not native.fpn_merge_supported(5, 64, torch.float32) and native.fpn_merge_supported(4, 64, SPLIT)


# ------------------------------------------------------------------------------------------------ RoIAlign over the levels
IMG = (96, 160)
MAPS = [(24, 40), (12, 20), (6, 10), (3, 5)]
SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
PH = PW = 7


def _rois(B=2, n=96, seed=96, fs=56):
    g = torch.Generator().manual_seed(seed)
    ih, iw = IMG
    side = (fs / 7.0) * torch.exp(torch.rand((n, 2), generator=g) * float(np.log(80.0)))      # fs / 7 .. 11 fs: every level
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([float(iw), float(ih)])
    box = torch.cat([ctr - side / 2, ctr + side / 2], 1)
    rois = torch.cat([torch.randint(0, B, (n, 1), generator=g).float(), box], 1)
    b = torch.from_numpy(R.boundary_boxes(x0=-20.0, y0=-30.0))
    rois[8:8 + len(b), 1:] = b
    rois[0, 1:] = torch.tensor([0., 0., iw - 1., ih - 1.])                # the whole image
    rois[1, 1:] = torch.tensor([50., 60., 50., 60.])                      # a single pixel
    rois[2, 1:] = torch.tensor([-200., -150., 80., 60.])                  # sticks out top-left
    rois[3, 1:] = torch.tensor([iw - 40., ih - 30., iw + 300., ih + 200.])  # sticks out bottom-right
    rois[4, 1:] = torch.tensor([120., 90., 40., 30.])                     # malformed, both sides negative: a positive product
    rois[5, 1:] = torch.tensor([120., 20., 40., 70.])                     # malformed, one side negative: the NaN scale, level 0
    rois[6] = torch.tensor([B - 1., 10., 10., 90., 70.])                  # batch index B - 1
    rois[7] = torch.tensor([B - 1., -300., -200., 500., 400.])
    return rois


def _feats(C, dtype, seed, B=2, maps=MAPS):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, h, w, C), generator=g).to(dtype).to(DEV) for h, w in maps]


def _per_level(feats, pool_rois, levels, sn, scales=SCALES):
    """native.roi_align_fwd per level, scattered: the rows every RoI must equal bit for bit."""
    K, C = pool_rois.shape[0], feats[0].shape[3]
    want = torch.zeros((K, PH, PW, C), dtype=feats[0].dtype, device=DEV)
    for l, f in enumerate(feats):
        ks = torch.nonzero(levels == l).flatten()
        if ks.numel():
            want[ks] = native.roi_align_fwd(f, pool_rois[ks].contiguous(), PH, PW, scales[l], sn, NHWC)
    return want


LEVEL_CASES = [(m, 64, 2, 56) for m in ('bf16', 'f16', 'f32')] + [('bf16', 24, 2, 14), ('f16', 64, 0, 14), ('f32', 12, 0, 56), ('f32', 24, 2, 14),
                                                                 ('bf16', 64, 0, 56)]


@pytest.mark.parametrize('mode,C,sn,fs', LEVEL_CASES)
def test_levels_rows_equal_the_single_level_call_and_the_statement(mode, C, sn, fs):
    dtype = DTYPES[mode]
    rois = _rois(fs=fs)
    lv_want = R.level_rule(rois.numpy(), fs, 4)
    assert set(lv_want.tolist()) == {0, 1, 2, 3} and lv_want[5] == 0
    assert float((rois[5, 3] - rois[5, 1] + 1) * (rois[5, 4] - rois[5, 2] + 1)) < 0          # the NaN scale: sqrt of a negative product
    feats = _feats(C, dtype, 31 * C + sn)
    K = rois.shape[0]
    n = K * PH * PW * C
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    d_rois = rois.to(DEV)
    out, lv = native.roi_align_levels(feats, d_rois, 7, SCALES, finest_scale=fs, sample_num=sn, with_levels=True, out=buf[:n].view(K, PH, PW, C))
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), 'guard elements behind the output were written'
    assert lv.dtype == torch.int32 and np.array_equal(lv.cpu().numpy(), lv_want)
    want = _per_level(feats, d_rois, lv, sn)
    nbad = int((bits(out) != bits(want)).sum())
    print('roi_align_levels %s C=%d sn=%d fs=%d: levels %s, %d of %d elements differ from the per-level call'
          % (mode, C, sn, fs, np.bincount(lv_want, minlength=4).tolist(), nbad, n))
    assert nbad == 0
    comp = native.roi_align_levels(feats, d_rois, 7, SCALES, finest_scale=fs, sample_num=sn, route='composite')
    assert same_bits(comp, out)
    # the per-level f64 statement and its bound (plus half an ulp of the storage format)
    ref, tol, nan = R.roi_levels_statement(rois, rois, lv_want, [f.float().cpu() for f in feats], PH, PW, SCALES, sn)
    got = out.double().cpu().view(K, PH * PW, C)
    assert torch.equal(torch.isnan(got).any(-1), nan) and torch.equal(torch.isnan(got).all(-1), nan)
    live = ~nan
    bound = tol + STORE_U[dtype] * (ref.abs() + tol) + STORE_ABS[dtype]
    ratio = ((got - ref).abs()[live] / bound[live].clamp(min=1e-300))
    ratio = torch.where((got - ref).abs()[live] == 0, torch.zeros_like(ratio), ratio)
    print('RATIO roi_align_levels:%s:C%d:s%d %.4g' % (mode, C, sn, float(ratio.max())))
    assert float(ratio.max()) <= 1.0


def test_levels_edge_calls():
    feats = _feats(64, torch.bfloat16, 7)
    rois = _rois().to(DEV)
    empty = native.roi_align_levels(feats, rois[:0], 7, SCALES)
    assert tuple(empty.shape) == (0, 7, 7, 64)
    lv = torch.from_numpy(R.level_rule(rois.cpu().numpy(), 56, 4)).to(DEV)
    for keep in ([1], [0, 3], [0, 1, 3]):                     # one level only; a middle level (two of them) left empty
        sel = rois[torch.isin(lv, torch.tensor(keep, device=DEV))].contiguous()
        out, l2 = native.roi_align_levels(feats, sel, 7, SCALES, with_levels=True)
        assert sorted(set(l2.tolist())) == keep
        assert same_bits(out, _per_level(feats, sel, l2, 2))
    two = native.roi_align_levels(feats[:2], rois, 7, SCALES[:2], with_levels=True)     # L = 2: the levels clamp
    assert np.array_equal(two[1].cpu().numpy(), R.level_rule(rois.cpu().numpy(), 56, 2))
    assert same_bits(two[0], _per_level(feats[:2], rois, two[1], 2))
    with pytest.raises(native.HvrError, match='no instance'):
        native.roi_align_levels([f[..., :6].contiguous() for f in feats], rois, 7, SCALES)


def test_levels_roi_scale_factor_and_split_half():
    """roi_scale_factor = 1.5: the levels come from the original boxes, the rescaled ones are pooled.  A split-half input equals the
    f32 call cast."""
    feats = _feats(64, torch.float32, 11)
    rois = _rois().to(DEV)
    out, lv = native.roi_align_levels(feats, rois, 7, SCALES, roi_scale_factor=1.5, with_levels=True)
    assert np.array_equal(lv.cpu().numpy(), R.level_rule(rois.cpu().numpy(), 56, 4))
    scaled = native.roi_rescale(rois, 1.5).contiguous()
    assert not np.array_equal(R.level_rule(scaled.cpu().numpy(), 56, 4), lv.cpu().numpy())      # the rescaled boxes would choose other levels
    assert same_bits(out, _per_level(feats, scaled, lv, 2))
    split = [native.cast(f, SPLIT) for f in feats]
    back = [native.cast(s, torch.float32) for s in split]
    got = native.roi_align_levels(split, rois, 7, SCALES)
    assert got.dtype == SPLIT and torch.equal(got, native.cast(native.roi_align_levels(back, rois, 7, SCALES), SPLIT))


# ------------------------------------------------------------------------------------------------ the FPN module
def _neck(name, gold, dtype):
    m = FPN(**R.CONFIGS[name])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.fixture_weights(gold, name).items()}, strict=True)
    m.eval().to(DEV)
    return set_compute_dtype(m, dtype)


def _hand_chain(m, xs):
    """forward as a chain of public native calls on the module's packed weights."""
    dt, p = m.compute_dtype, m.packed(torch.device(DEV))
    relu, split = m.activation == 'relu', m.compute_dtype == SPLIT
    conv = lambda x, wb, **kw: native.conv2d_nhwc(kstep_pad(x, wb[0].shape[-1]), wb[0], wb[1], relu=relu, **kw)
    n = len(m.lateral_convs)
    lat = [conv(xs[i + m.start_level], p['lateral'][i], out_f32=split) for i in range(n)]
    merged = native.fpn_merge(lat)
    if split:
        merged = [native.cast(t, SPLIT) for t in merged]
    outs = [conv(merged[i], p['fpn'][i], pad=1) for i in range(n)]
    if m.num_outs > n and not m.add_extra_convs:
        for _ in range(m.num_outs - n):
            outs.append(outs[-1][:, ::2, ::2].contiguous())
    elif m.num_outs > n:
        outs.append(conv(xs[m.backbone_end_level - 1] if m.extra_convs_on_inputs else outs[-1], p['fpn'][n], stride=2, pad=1))
        for i in range(n + 1, m.num_outs):
            outs.append(conv(torch.relu(outs[-1]) if m.relu_before_extra_convs else outs[-1], p['fpn'][i], stride=2, pad=1))
    return outs


@pytest.fixture(scope='module')
def gold():
    return R.golden()


@pytest.mark.parametrize('mode', ['bf16', 'f16', 'f16x2', 'f32'])
@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_fpn_forward_equals_the_hand_made_chain(gold, name, mode):
    dtype = dict(DTYPES, f16x2=SPLIT)[mode]
    m = _neck(name, gold, dtype)
    inputs = [torch.from_numpy(x).to(DEV) for x in R.fixture_inputs(gold)]
    outs = m(inputs)
    chain = _hand_chain(m, [as_nhwc(x, dtype) for x in inputs])
    want_shapes = [o.shape for o in R.fixture_outs(gold, name)]
    assert [tuple(o.shape) for o in outs] == [tuple(s) for s in want_shapes]
    for o, c in zip(outs, chain):
        assert o.dtype == dtype and torch.equal(o.permute(0, 2, 3, 1), c)
        assert o.permute(0, 2, 3, 1).is_contiguous()                       # logical NCHW over physical NHWC
    if dtype != SPLIT:
        assert all(bool(torch.isfinite(o.float()).all()) and float(o.float().abs().max()) > 0 for o in outs)


@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_fpn_f32_meets_the_reference_within_the_forward_error_bound(gold, name):
    m = _neck(name, gold, torch.float32)
    outs = m([torch.from_numpy(x).to(DEV) for x in R.fixture_inputs(gold)])
    want = R.fixture_outs(gold, name)
    bound = R.fpn_bound(R.fixture_inputs(gold), R.fixture_weights(gold, name), R.CONFIGS[name])
    worst = 0.0
    for o, w, b in zip(outs, want, bound):
        err = np.abs(o.double().cpu().numpy() - w)
        worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    print('RATIO fpn_forward:%s f32 %.4g (largest bound %.3g on outputs up to %.3g)' % (name, worst, max(float(b.max()) for b in bound),
                                                                                    max(float(np.abs(w).max()) for w in want)))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the extractor on the golden maps
def test_extractor_on_the_golden_maps(gold):
    """Levels exact; every element within the RoIAlign bound of the oracle's f32 outputs (the oracle's own f32 evaluation lies within
    the same bound of the f64 statement: twice the bound between the two)."""
    ext = SingleRoIExtractor(dict(type='RoIAlign', out_size=7, sample_num=2), 8, [4, 8, 16, 32], finest_scale=56)
    feats = [torch.from_numpy(gold['ext.feat%d' % i]).to(DEV).contiguous(memory_format=torch.channels_last) for i in range(4)]
    rois = torch.from_numpy(gold['ext.rois'])
    maps = [f.permute(0, 2, 3, 1) for f in feats]
    _, lv = native.roi_align_levels(maps, rois.to(DEV), 7, [1 / 4, 1 / 8, 1 / 16, 1 / 32], with_levels=True)
    assert np.array_equal(lv.cpu().numpy(), gold['ext.levels'])
    for key, sel, factor in (('ext.out', slice(None), None), ('ext.out_rescaled', slice(0, 32), 1.5)):
        r = rois[sel]
        got = ext(feats, r.to(DEV), roi_scale_factor=factor)
        assert tuple(got.shape) == gold[key].shape
        pool = native.roi_rescale(r, factor) if factor else r
        ref, tol, nan = R.roi_levels_statement(r, pool, gold['ext.levels'][sel], [m.cpu() for m in maps], 7, 7, [1 / 4, 1 / 8, 1 / 16, 1 / 32], 2)
        assert not bool(nan.any())
        K = r.shape[0]
        g = got.permute(0, 2, 3, 1).reshape(K, 49, 8).double().cpu()
        o = torch.from_numpy(gold[key]).permute(0, 2, 3, 1).reshape(K, 49, 8).double()
        assert float(((g - ref).abs() / tol.clamp(min=1e-300)).max()) <= 1.0
        ratio = float(((g - o).abs() / (2 * tol).clamp(min=1e-300)).max())
        print('RATIO extractor:%s %.4g' % (key, ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ the whole path
def test_r50_fpn_extractor_whole_path_and_graph():
    det = TwoStageDetector(backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch'),
                           neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5))
    ext = SingleRoIExtractor(dict(type='RoIAlign', out_size=7, sample_num=2), 256, [4, 8, 16, 32])
    det.eval().to(DEV)
    g = torch.Generator().manual_seed(3)
    img = torch.randn((2, 3, 64, 96), generator=g).to(DEV)
    with torch.no_grad():
        c = det.backbone(img)
        feats = det.extract_feat(img)
    assert [tuple(f.shape) for f in feats] == [(2, 256, 16, 24), (2, 256, 8, 12), (2, 256, 4, 6), (2, 256, 2, 3), (2, 256, 1, 2)]
    for f in feats:
        assert bool(torch.isfinite(f.float()).all()) and float(f.float().abs().max()) > 0
    rois = _rois(fs=14)
    rois[:, 1:] *= 0.6
    rois = rois.to(DEV)
    with torch.no_grad():
        eager = ext(feats, rois)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ext(det.neck(c), rois)                           # the side stream's workspaces and its view of the packed weights
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):       # capture fails if anything reads the host
                cap_feats = det.neck(c)
                cap = ext(cap_feats, rois)
        torch.cuda.current_stream().wait_stream(side)
        cap.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
    assert tuple(eager.shape) == (96, 256, 7, 7) and float(eager.float().abs().max()) > 0
    assert torch.equal(cap, eager)
    for a, b in zip(cap_feats, feats):
        assert torch.equal(a, b)
