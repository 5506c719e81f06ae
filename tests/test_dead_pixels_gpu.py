"""The backbone skips the pixels that the stride-2 stages never read (ResNet.skip_dead_pixels).

A caffe-style stage puts its stride on the first block's 1x1 conv1 and 1x1 downsample (mmdet/models/backbones/resnet.py:127-132,
283-296), so the stage before it is read at pixels (2 oy, 2 ox) only.  Its last block then runs conv2 as a stride-2 3x3 and the
closing 1x1 + residual on the compact map, the residual sampled from the block's full-resolution input
(hvr_bottleneck_close_sampled).  Nothing here has a tolerance: every per-pixel sum keeps its MFMA order, so every comparison is
torch.equal / np.array_equal against the full-resolution path.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
MODES = [torch.bfloat16, torch.float16, SPLIT]
MODE_IDS = ['bf16', 'half', 'split_half']
# (B, RH, RW): odd sizes -- 280 output rows = two 128-row panels and a ragged one, a frame boundary inside a panel; even sizes -- the
# last row and column are never read; 30 output rows -- fewer than one panel
SIZES = [(2, 19, 27), (3, 20, 26), (1, 9, 11)]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _to(x, dtype):
    return native.cast(x.to(DEV).contiguous(), dtype)


def _back(y):
    return native.cast(y, torch.float32) if y.dtype != torch.float32 else y


def _sentinel(shape, dtype):
    if dtype == SPLIT:
        return torch.full(shape, 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    return torch.full(shape, 123.0, dtype=dtype, device=DEV)


@pytest.mark.parametrize('dt', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('B,RH,RW', SIZES)
@pytest.mark.parametrize('C1,Cout', [(64, 256), (128, 512)])
def test_sampled_close_equals_the_full_close_at_even_pixels(C1, Cout, B, RH, RW, dt):
    """hvr_bottleneck_close_sampled against hvr_conv2d_nhwc on the full map, sliced [:, ::2, ::2]: bit-identical; only the sampled
    residual pixels are read (every other one is NaN in a second pass); nothing is written behind row M."""
    OH, OW = (RH - 1) // 2 + 1, (RW - 1) // 2 + 1
    M = B * OH * OW
    h_full = _to(_rand((B, RH, RW, C1), 1), dt)
    x32 = _rand((B, RH, RW, Cout), 2)
    x = _to(x32, dt)
    w3, b3 = native.as_operand(_rand((Cout, C1), 3, 0.1).to(DEV), dt), _rand((Cout,), 4, 0.1).to(DEV)
    ref = native.conv2d_nhwc(h_full, w3.view(Cout, 1, 1, C1), b3, resid=x, relu=True)[:, ::2, ::2]
    h = h_full[:, ::2, ::2].contiguous()
    assert tuple(h.shape) == (B, OH, OW, C1)
    if not native.bottleneck_close_sampled_supported(h, w3, b3, x, 2):
        # fewer rows than one 128-row panel: the query says no, the call refuses (no quiet other kernel), and the caller keeps the
        # full-resolution block (test_last_block_of_a_stage_on_the_live_pixels)
        assert M < 128
        with pytest.raises(native.HvrError):
            native.bottleneck_close_sampled(h, w3, b3, x, stride=2)
        return
    assert M >= 128
    whole = _sentinel((M + 64, Cout), dt)
    y = native.bottleneck_close_sampled(h, w3, b3, x, stride=2, out=whole[:M].view(B, OH, OW, Cout))
    assert torch.equal(y, ref)
    assert torch.equal(whole[M:], _sentinel((64, Cout), dt))
    # second pass: every residual pixel with an odd row or column (for even sizes that covers the last row / column) is NaN
    xn = x32.clone()
    xn[:, 1::2] = float('nan')
    xn[:, :, 1::2] = float('nan')
    if RH % 2 == 0:
        xn[:, RH - 1] = float('nan')
    if RW % 2 == 0:
        xn[:, :, RW - 1] = float('nan')
    y2 = native.bottleneck_close_sampled(h, w3, b3, _to(xn, dt), stride=2)
    assert torch.equal(y2, ref)
    assert torch.isfinite(_back(y2)).all()


def test_sampled_close_has_no_exact_f32_kernel():
    """exact f32 runs on the tile engine, which has no sampled-residual epilogue: the query says so and the block stays at full resolution."""
    h, x = _rand((2, 10, 14, 64), 5).to(DEV), _rand((2, 19, 27, 256), 6).to(DEV)
    assert not native.bottleneck_close_sampled_supported(h, _rand((256, 64), 7, 0.1).to(DEV), _rand((256,), 8).to(DEV), x, 2)
    # sampled pixels outside the residual map
    hb, xb = _to(_rand((2, 10, 14, 64), 5), torch.bfloat16), _to(_rand((2, 18, 27, 256), 6), torch.bfloat16)
    assert not native.bottleneck_close_sampled_supported(hb, _rand((256, 64), 7, 0.1).to(DEV).bfloat16(), _rand((256,), 8).to(DEV), xb, 2)


@pytest.mark.parametrize('dt', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('B,RH,RW', SIZES)
@pytest.mark.parametrize('C', [64, 128])
def test_stride2_conv3x3_equals_the_stride1_conv_at_even_pixels(C, B, RH, RW, dt):
    """No new kernel: the dispatch equality the elimination rests on (64 -> 64 at stride 1 is the persistent LDS-resident kernel on
    large maps, at stride 2 the tile engine)."""
    h = _to(_rand((B, RH, RW, C), 11), dt)
    w, b = native.as_operand(_rand((C, 3, 3, C), 12, 0.05).to(DEV), dt), _rand((C,), 13, 0.1).to(DEV)
    full = native.conv2d_nhwc(h, w, b, relu=True, stride=1, pad=1)
    half = native.conv2d_nhwc(h, w, b, relu=True, stride=2, pad=1)
    assert tuple(half.shape) == (B, (RH - 1) // 2 + 1, (RW - 1) // 2 + 1, C)
    assert torch.equal(half, full[:, ::2, ::2])


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'half'])
def test_stride2_conv3x3_c64_on_a_map_the_persistent_kernel_takes(dt):
    """2 x 53 x 75 pixels: the stride-1 conv is the persistent 64 -> 64 kernel (hvr_conv2d_path 2), the stride-2 one is not."""
    B, H, W, C = 2, 53, 75, 64
    assert native.conv2d_path(B, H, W, C, C, k=3, stride=1, pad=1, dtype=dt, resid=False) == 2
    assert native.conv2d_path(B, H, W, C, C, k=3, stride=2, pad=1, dtype=dt, resid=False) != 2
    h = _to(_rand((B, H, W, C), 14), dt)
    w, b = native.as_operand(_rand((C, 3, 3, C), 15, 0.05).to(DEV), dt), _rand((C,), 16, 0.1).to(DEV)
    assert torch.equal(native.conv2d_nhwc(h, w, b, relu=True, stride=2, pad=1), native.conv2d_nhwc(h, w, b, relu=True, stride=1, pad=1)[:, ::2, ::2])


def _backbone_state(depth_blocks, seed):
    """Seeded weights and BatchNorm statistics with LIVE residual branches (gamma = 0 makes them dead)."""
    from hvrnet_amd import synthetic as S
    g = torch.Generator().manual_seed(seed)
    sd = {'conv1.weight': S._conv(g, 64, 3, 7)}
    S._bn(g, sd, 'bn1', 64)
    inplanes = 64
    for i, nb in enumerate(depth_blocks):
        S._res_layer(g, sd, 'layer%d' % (i + 1), inplanes, 64 * 2 ** i, nb)
        inplanes = 64 * 2 ** i * 4
    return sd


def _resnet(style='caffe', out_indices=(2,)):
    from hvrnet_amd.backbone import ResNet
    net = ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=out_indices, style=style, zero_init_residual=False)
    net.load_state_dict(_backbone_state((3, 4, 6), 7))
    return net.to(DEV)


_NETS = {}


def _net(style='caffe', out_indices=(2,)):
    key = (style, out_indices)
    if key not in _NETS:
        _NETS[key] = _resnet(style, out_indices)
    return _NETS[key]


def _frames(B, H, W):
    from hvrnet_amd import synthetic as S
    return torch.cat([S.synth_frame(i, img_hw=(H, W), pad_hw=(H, W)) for i in range(B)]).to(DEV)


class _Counted(object):
    """native.bottleneck_close_sampled behind a call counter."""

    def __init__(self, monkeypatch):
        self.calls = 0
        real = native.bottleneck_close_sampled

        def wrapper(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(native, 'bottleneck_close_sampled', wrapper)


BOTH = (0, 1)   # ResNet.compact_stages with layer 2 in it as well (the default keeps layer 2 full: see the attribute)


def _on_off(net, x, monkeypatch, counted, stages=BOTH):
    from hvrnet_amd.backbone import ResNet
    monkeypatch.setattr(ResNet, 'compact_stages', stages)
    with torch.no_grad():
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
        off = [o.clone() for o in net(x)]
        assert counted.calls == 0
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', True)
        on = [o.clone() for o in net(x)]
    return on, off


@pytest.mark.parametrize('dt', MODES + [torch.float32], ids=MODE_IDS + ['f32'])
@pytest.mark.parametrize('shape', [(2, 3, 212, 300), (1, 3, 200, 296)], ids=['2x212x300', '1x200x296'])
@pytest.mark.parametrize('stages', [BOTH, (0,)], ids=['layers_1_2', 'default'])
def test_backbone_c4_is_bit_identical_with_the_dead_pixels_skipped(stages, shape, dt, monkeypatch):
    """Stage maps 53x75 -> 27x38 -> 14x19 and 50x74 -> 25x37 -> 13x19: C4 with the attribute on equals C4 with it off (the parent's
    path) bit for bit; two sampled closes per forward with layers 1 and 2 compact, one with the default (layer 1 only), none in
    exact f32 (no kernel: the stages stay full)."""
    from hvrnet_amd.backbone import set_compute_dtype
    net = set_compute_dtype(_net(), dt)
    counted = _Counted(monkeypatch)
    x = _frames(shape[0], shape[2], shape[3])
    from hvrnet_amd.backbone import ResNet
    assert ResNet.skip_dead_pixels is True and ResNet.compact_stages == (0,)
    on, off = _on_off(net, x, monkeypatch, counted, stages)
    assert counted.calls == (0 if dt == torch.float32 else len(stages))
    assert len(on) == len(off) == 1 and on[0].shape == off[0].shape
    assert tuple(on[0].shape) == (shape[0], 1024) + {212: (14, 19), 200: (13, 19)}[shape[2]]
    assert torch.equal(on[0], off[0])
    assert torch.isfinite(_back(on[0].permute(0, 2, 3, 1).contiguous())).all()


def test_backbone_one_frame_under_fewrow_split(monkeypatch):
    """Few-row split-K picks its K slices by the row count, so a compact 3x3 would sum in another order than the full one: the
    elimination is gated off there (no sampled close), and C4 is the same either way."""
    from hvrnet_amd.backbone import set_compute_dtype
    net = set_compute_dtype(_net(), torch.bfloat16)
    counted = _Counted(monkeypatch)
    x = _frames(1, 212, 300)
    with native.fewrow_split(True):
        on, off = _on_off(net, x, monkeypatch, counted)
    assert counted.calls == 0
    assert torch.equal(on[0], off[0])


@pytest.mark.parametrize('style,out_indices', [('pytorch', (2,)), ('caffe', (0, 1, 2))], ids=['pytorch_style', 'every_stage_returned'])
def test_backbone_keeps_full_resolution_where_the_pixels_are_read(style, out_indices, monkeypatch):
    """style='pytorch' puts the stride on the 3x3 (every pixel is read); a returned stage map is read by the caller."""
    from hvrnet_amd.backbone import set_compute_dtype
    net = set_compute_dtype(_net(style, out_indices), torch.bfloat16)
    counted = _Counted(monkeypatch)
    x = _frames(2, 212, 300)
    on, off = _on_off(net, x, monkeypatch, counted)
    assert counted.calls == 0
    assert len(on) == len(off) == len(out_indices)
    want = {0: (53, 75), 1: (27, 38), 2: (14, 19)}
    for i, a, b in zip(out_indices, on, off):
        assert tuple(a.shape[2:]) == want[i] and torch.equal(a, b)


@pytest.mark.parametrize('dt', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('B,H,W', SIZES)
def test_last_block_of_a_stage_on_the_live_pixels(B, H, W, dt, monkeypatch):
    """Bottleneck.close_sampled = forward_nhwc at [:, ::2, ::2]; below one 128-row panel the route (ResNet.stage_route, without the
    live-store form in front) says the full-resolution close, which returns the full map."""
    from hvrnet_amd.backbone import ResNet, set_compute_dtype
    net = _net()
    blk = set_compute_dtype(net.layer1[2], dt)
    monkeypatch.setattr(ResNet, 'live_store_stages', ())
    step = net.stage_route(0, B, H, W, dt).steps[-1]
    compact = (step.kind, step.stride) == ('close_sampled', 2)
    x = _to(_rand((B, H, W, 256), 21).abs(), dt)
    with torch.no_grad():
        full = blk.forward_nhwc(x)
        y = blk.close_sampled(x) if compact else blk.close(x, blk.body(x), step)
    assert compact == (B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) >= 128)
    assert torch.equal(y, full[:, ::2, ::2] if compact else full)


@pytest.mark.parametrize('stages', [BOTH, (0,)], ids=['layers_1_2', 'default'])
def test_window_detections_do_not_change(stages, monkeypatch):
    """One small HVR window end to end (320 x 512, T = 3, bf16 and split half): every per-class array is the same with the attribute
    on and off."""
    import hvrnet_amd
    from hvrnet_amd import synthetic as S
    from hvrnet_amd.backbone import ResNet
    from hvrnet_amd.config import hvr_config
    T, hw, pad = 3, (310, 500), (320, 512)
    imgs = [S.synth_frame(i, img_hw=hw, pad_hw=pad) for i in range(T)]
    metas = [S.synth_meta(hw, pad) for _ in range(T)]
    model = hvrnet_amd.build_model(hvr_config(frame_interval=1, nms_post=16), S.synth_state_dict('hvr'), torch.bfloat16, DEV)
    counted = _Counted(monkeypatch)
    monkeypatch.setattr(ResNet, 'compact_stages', stages)

    def run():
        with torch.no_grad():
            c4 = [model(img=im.to(DEV), img_meta=[m], backbone_feat=True)[0] for im, m in zip(imgs, metas)]
            return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)

    for dt in (torch.bfloat16, SPLIT):
        hvrnet_amd.set_compute_dtype(model, dt)
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
        off = run()
        assert counted.calls == 0
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', True)
        on = run()
        assert counted.calls == len(stages) * T
        counted.calls = 0
        n = 0
        for b in range(len(off)):
            assert len(on[b]) == len(off[b])
            for c in range(len(off[b])):
                assert np.array_equal(np.asarray(on[b][c]), np.asarray(off[b][c])), (native.DTYPE_NAMES[dt], b, c)
                n += len(np.asarray(off[b][c]))
        assert n > 0
