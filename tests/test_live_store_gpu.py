"""The block before the last of a stage that ends compact writes only the live quarter of its output
(hvr_bottleneck_tail_next_live, ResNet.live_store_stages).

The last block of such a stage reads its input map twice: conv1 -- which the block before computes from registers -- and the
residual, which the stride-2 consumer's pixels (2 oy, 2 ox) need and no other.  The live-store form of the fused tail + next conv1
computes every pixel as before and stores y at the live pixels only, as a compact map; a dead pixel's lanes are masked out of the
store instruction, which every wave still issues, so the kernel's vmcnt counts hold.  Same MFMA order, same bits: every comparison with the
plain form is torch.equal / np.array_equal; the f64 statement and bound are those of tests/forward_kernel_refs.py.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native  # noqa: E402
from tests import forward_kernel_refs as R  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
MODES = [torch.bfloat16, torch.float16, SPLIT]
MODE_IDS = ['bf16', 'half', 'split_half']
GUARD = 64          # sentinel rows in front of and behind every output
# [B, H, W]: odd H and W, M = 494 -- a ragged last panel and a frame boundary inside a panel; even H and W (the last row and column are
# dead); M = 135 -- two panels, the second of 7 rows
MAPS = [(2, 13, 19), (2, 14, 20), (1, 9, 15)]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _to(x, dtype):
    return native.cast(x.to(DEV).contiguous(), dtype)


def _fill(dtype):
    return 0x5a5a5a5a if dtype == SPLIT else 123.0


def _guarded(rows, cols, dtype):
    """(the [rows, cols] view to write into, the whole sentinel-filled buffer with GUARD rows at both ends)"""
    buf = torch.full((rows + 2 * GUARD, cols), _fill(dtype), dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + rows], buf


def _guards_intact(buf, rows):
    return bool((buf[:GUARD] == _fill(buf.dtype)).all()) and bool((buf[GUARD + rows:] == _fill(buf.dtype)).all())


def _operands(B, H, W, C1, Cout, Cn, dt, seed=0):
    h = _to(_rand((B, H, W, C1), seed + 1).clamp(min=0.0), dt)
    resid = _to(_rand((B, H, W, Cout), seed + 2).clamp(min=0.0), dt)
    w3 = native.as_operand(_rand((Cout, C1), seed + 3, C1 ** -0.5).to(DEV), dt)
    b3 = _rand((Cout,), seed + 4, 0.1).to(DEV)
    wn = native.as_operand(_rand((Cn, Cout), seed + 5, Cout ** -0.5).to(DEV), dt)
    bn = _rand((Cn,), seed + 6, 0.1).to(DEV)
    return h, resid, w3, b3, wn, bn


@pytest.mark.parametrize('dt', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('B,H,W', MAPS)
@pytest.mark.parametrize('C1,Cout,Cn', [(64, 256, 64), (128, 512, 128)])
def test_live_store_equals_the_plain_form_at_the_live_pixels(C1, Cout, Cn, B, H, W, dt):
    """y_live = bottleneck_tail_next(...)[0][:, ::2, ::2] and hn = its hn, bit for bit; nothing is written outside y_live and hn
    (sentinel rows in front of and behind each; the kernel has no other output: the dead pixels are not stored anywhere); both outputs
    lie inside the f64 statement's bracket, every element."""
    if dt == SPLIT and Cout != 256:
        assert not native.tail_next_live_path(B, H, W, C1, Cout, Cn, 2, SPLIT)   # expand_split.hip has no other next-form
        return
    h, resid, w3, b3, wn, bn = _operands(B, H, W, C1, Cout, Cn, dt)
    assert native.bottleneck_tail_next_live_supported(h, resid, w3, b3, wn, bn, 2)
    y_ref, hn_ref = native.bottleneck_tail_next(h, None, resid, w3, b3, wn, bn)
    LH, LW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ML, M = B * LH * LW, B * H * W
    yv, ybuf = _guarded(ML, Cout, dt)
    hv, hbuf = _guarded(M, Cn, dt)
    y_live, hn = native.bottleneck_tail_next_live(h, resid, w3, b3, wn, bn, live_stride=2, out=yv.view(B, LH, LW, Cout), out_hn=hv.view(B, H, W, Cn))
    torch.cuda.synchronize()
    assert torch.equal(y_live, y_ref[:, ::2, ::2])
    assert torch.equal(hn, hn_ref)
    assert _guards_intact(ybuf, ML) and _guards_intact(hbuf, M)
    # without caller-owned outputs: the same maps
    y2, hn2 = native.bottleneck_tail_next_live(h, resid, w3, b3, wn, bn, live_stride=2)
    assert torch.equal(y2, y_live) and torch.equal(hn2, hn)
    # the f64 statement of the fused tail + next conv1 (tests/forward_kernel_refs.py), every element inside its bracket
    mode = R.mode_of(dt)
    wv, wnv = R.values(w3, 'weight'), R.values(wn, 'weight')
    t = R.tail_next_statement(R.values(h), None, R.values(resid), wv, b3, wnv, bn, 1, mode)
    ref, mag, absxw = t['y']
    lo, hi = R.stored_bracket(ref, R.mfma_bound(mag, absxw, C1, mode), mode)
    ratio, bad, _ = R.compare(R.values(y_live), lo[:, ::2, ::2], hi[:, ::2, ::2], ref[:, ::2, ::2])
    print('RATIO live.y %s %.4g' % (mode, ratio))
    assert bad == 0, (bad, ratio)
    href, hmag, habs = t['hn']
    hb = R.mfma_bound(hmag, habs, Cout, mode) + R.hn_extra(lo, hi, t['y_stored'], wnv)
    hlo, hhi = R.stored_bracket(href, hb, mode)
    ratio, bad, _ = R.compare(R.values(hn), hlo, hhi, href)
    print('RATIO live.hn %s %.4g' % (mode, ratio))
    assert bad == 0, (bad, ratio)


def test_live_store_has_no_kernel_for_other_blocks():
    """Layer 3's (1024, 256), exact f32 and a projection block: the query says 0 and the call refuses."""
    B, H, W = 2, 13, 19
    assert not native.tail_next_live_path(B, H, W, 256, 1024, 256, 2, torch.bfloat16)
    assert not native.tail_next_live_path(512, 38, 63, 256, 1024, 256, 2, torch.bfloat16)   # (the plain form runs there: 512 panels and more)
    assert not native.tail_next_live_path(B, H, W, 64, 256, 64, 2, torch.float32)
    h, resid, w3, b3, wn, bn = _operands(B, H, W, 64, 256, 64, torch.bfloat16)
    assert not native.bottleneck_tail_next_live_supported(h.float(), resid.float(), w3.float(), b3, wn.float(), bn, 2)
    assert native.bottleneck_tail_next_live_supported(h, resid, w3, b3, wn, bn, 2)
    # a projection block: tail.C2 > 0 (x = the block input, no residual)
    x = _to(_rand((B, H, W, 64), 9), torch.bfloat16)
    wt = native.as_operand(_rand((256, 128), 10, 0.1).to(DEV), torch.bfloat16)
    assert native.bottleneck_tail_next_supported(h, x, None, wt, b3, 1, wn, bn)
    y, hn = torch.empty((B, 7, 10, 256), dtype=torch.bfloat16, device=DEV), torch.empty((B, H, W, 64), dtype=torch.bfloat16, device=DEV)
    d = native.TailNextLiveDesc(next=native._tail_next_desc(h, x, None, wt, b3, 1, wn, bn, y, hn), live_stride=2)
    assert native.lib().hvr_bottleneck_tail_next_live_supported(ctypes.byref(d)) == 0
    assert native.lib().hvr_bottleneck_tail_next_live(ctypes.byref(d), native._stream()) != 0
    # a stride of 0
    d = native._tail_next_live_desc(h, resid, w3, b3, wn, bn, 0, y, hn)
    assert native.lib().hvr_bottleneck_tail_next_live_supported(ctypes.byref(d)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the stages
def _backbone_state(depth_blocks, seed):
    """Seeded weights and BatchNorm statistics with live residual branches (as tests/test_dead_pixels_gpu.py)."""
    from hvrnet_amd import synthetic as S
    g = torch.Generator().manual_seed(seed)
    sd = {'conv1.weight': S._conv(g, 64, 3, 7)}
    S._bn(g, sd, 'bn1', 64)
    inplanes = 64
    for i, nb in enumerate(depth_blocks):
        S._res_layer(g, sd, 'layer%d' % (i + 1), inplanes, 64 * 2 ** i, nb)
        inplanes = 64 * 2 ** i * 4
    return sd


_NET = []


def _net():
    if not _NET:
        from hvrnet_amd.backbone import ResNet
        net = ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', zero_init_residual=False)
        net.load_state_dict(_backbone_state((3, 4, 6), 7))
        _NET.append(net.to(DEV))
    return _NET[0]


def _frames(B, H, W):
    from hvrnet_amd import synthetic as S
    return torch.cat([S.synth_frame(i, img_hw=(H, W), pad_hw=(H, W)) for i in range(B)]).to(DEV)


class _Calls(object):
    """Counters on the entries a stage can close through; conv2d_nhwc calls are kept by (output map, residual given)."""

    def __init__(self, monkeypatch):
        self.live, self.sampled, self.sampled_strides, self.convs = 0, 0, [], []
        real_live, real_sampled, real_conv = native.bottleneck_tail_next_live, native.bottleneck_close_sampled, native.conv2d_nhwc

        def live(*a, **k):
            self.live += 1
            return real_live(*a, **k)

        def sampled(h, w, bias, resid, stride=2, relu=True, out=None):
            self.sampled += 1
            self.sampled_strides.append(stride)
            return real_sampled(h, w, bias, resid, stride=stride, relu=relu, out=out)

        def conv(x, w, bias=None, resid=None, *a, **k):
            y = real_conv(x, w, bias, resid, *a, **k)
            if resid is not None and w.shape[1] == 1:
                self.convs.append((tuple(y.shape[1:]), tuple(resid.shape[1:])))
            return y
        monkeypatch.setattr(native, 'bottleneck_tail_next_live', live)
        monkeypatch.setattr(native, 'bottleneck_close_sampled', sampled)
        monkeypatch.setattr(native, 'conv2d_nhwc', conv)

    def reset(self):
        self.live, self.sampled, self.sampled_strides, self.convs = 0, 0, [], []


def _c4(net, x):
    with torch.no_grad():
        return [o.clone() for o in net(x)]


@pytest.mark.parametrize('dt', MODES + [torch.float32], ids=MODE_IDS + ['f32'])
@pytest.mark.parametrize('shape', [(2, 3, 212, 300), (1, 3, 200, 296)], ids=['2x212x300', '1x200x296'])
def test_backbone_c4_is_bit_identical_with_live_stores(shape, dt, monkeypatch):
    """Stage maps 53x75 -> 27x38 -> 14x19 and 50x74 -> 25x37 -> 13x19 on the defaults: C4 equals C4 with skip_dead_pixels off bit for
    bit.  bf16 / half: both stages run the live-store form, layer 1 closes through the sampled close at stride 1 (once), layer 2 through
    one conv2d_nhwc on the compact 27x38 / 25x37 map.  Split half: layer 1 only (no (512, 128) kernel), layer 2 stays full.  f32: none."""
    from hvrnet_amd.backbone import ResNet, set_compute_dtype
    assert ResNet.compact_stages == (0,) and ResNet.live_store_stages == (0, 1) and ResNet.skip_dead_pixels is True
    net = set_compute_dtype(_net(), dt)
    x = _frames(shape[0], shape[2], shape[3])
    calls = _Calls(monkeypatch)
    monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
    off = _c4(net, x)
    assert calls.live == 0 and calls.sampled == 0
    full2, compact2 = {212: ((27, 38), (14, 19)), 200: ((25, 37), (13, 19))}[shape[2]]
    closes_off = [c for c in calls.convs if c[0][2] == 512]
    assert closes_off and all(c[0][:2] == full2 for c in closes_off)
    calls.reset()
    monkeypatch.setattr(ResNet, 'skip_dead_pixels', True)
    on = _c4(net, x)
    assert len(on) == len(off) == 1 and torch.equal(on[0], off[0])
    closes = [c for c in calls.convs if c[0][2] == 512]    # layer 2's closing convs that went through conv2d_nhwc
    if dt == torch.float32:
        assert calls.live == 0 and calls.sampled == 0 and closes == closes_off
    elif dt == SPLIT:
        assert calls.live == 1 and calls.sampled == 1 and calls.sampled_strides == [1]
        assert closes == closes_off                                    # layer 2 stays at full resolution
    else:
        assert calls.live == 2 and calls.sampled == 1 and calls.sampled_strides == [1]
        assert closes == [(compact2 + (512,), compact2 + (512,))]      # one dense close on the compact map


@pytest.mark.parametrize('how', ['fuse_next_off', 'fewrow_split', 'no_live_store_stages'])
def test_backbone_keeps_the_earlier_call_pattern_where_the_form_is_off(how, monkeypatch):
    """Bottleneck.fuse_next = False, native.fewrow_split(True) and live_store_stages = () each give the call pattern from before the
    live-store form: no live call; layer 1 closes through the stride-2 sampled close (not under few-row split-K: full resolution
    there); layer 2 stays full.  C4 is unchanged."""
    import contextlib
    from hvrnet_amd.backbone import Bottleneck, ResNet, set_compute_dtype
    net = set_compute_dtype(_net(), torch.bfloat16)
    x = _frames(1, 212, 300)
    calls = _Calls(monkeypatch)
    ctx = contextlib.nullcontext()
    if how == 'fuse_next_off':
        monkeypatch.setattr(Bottleneck, 'fuse_next', False)
    elif how == 'fewrow_split':
        ctx = native.fewrow_split(True)
    else:
        monkeypatch.setattr(ResNet, 'live_store_stages', ())
    with ctx:
        got = _c4(net, x)
        live, strides, closes = calls.live, list(calls.sampled_strides), [c for c in calls.convs if c[0][2] == 512]
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
        want = _c4(net, x)
    assert live == 0
    assert strides == ([] if how == 'fewrow_split' else [2])
    assert closes and all(c[0][:2] == (27, 38) for c in closes)
    assert torch.equal(got[0], want[0])


def test_window_detections_do_not_change(monkeypatch):
    """One small HVR window end to end (320 x 512, T = 3, bf16 and split half): every per-class array is the same with
    skip_dead_pixels on (live stores included) and off; a GraphedClip replay equals the eager result."""
    import hvrnet_amd
    from hvrnet_amd import graphs, synthetic as S
    from hvrnet_amd.backbone import ResNet
    from hvrnet_amd.config import hvr_config
    T, hw, pad = 3, (310, 500), (320, 512)
    imgs = [S.synth_frame(i, img_hw=hw, pad_hw=pad) for i in range(T)]
    metas = [S.synth_meta(hw, pad) for _ in range(T)]
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=16), S.synth_state_dict('hvr'), torch.bfloat16, DEV)
    calls = _Calls(monkeypatch)

    def run():
        with torch.no_grad():
            c4 = [model(img=im.to(DEV), img_meta=[m], backbone_feat=True)[0] for im, m in zip(imgs, metas)]
            return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)

    def same(a, b, what):
        n = 0
        assert len(a) == len(b)
        for br in range(len(b)):
            assert len(a[br]) == len(b[br])
            for c in range(len(b[br])):
                assert np.array_equal(np.asarray(a[br][c]), np.asarray(b[br][c])), (what, br, c)
                n += len(np.asarray(b[br][c]))
        assert n > 0

    for dt in (torch.bfloat16, SPLIT):
        hvrnet_amd.set_compute_dtype(model, dt)
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
        off = run()
        assert calls.live == 0
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', True)
        on = run()
        assert calls.live == (2 if dt == torch.bfloat16 else 1) * T and calls.sampled == T
        calls.reset()
        same(on, off, native.DTYPE_NAMES[dt])
    # the captured clip (one hipGraph of the whole window) replays to the eager result
    hvrnet_amd.set_compute_dtype(model, torch.bfloat16)
    batch = torch.cat(imgs).to(DEV)
    with torch.no_grad():
        c4 = model(img=batch, img_meta=metas, backbone_feat=True)[0]
        eager = model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
    clip = graphs.GraphedClip(model, batch, metas, rescale=True)
    for what in ('graph', 'graph replay'):
        same(clip.run(batch).result(), eager, what)
