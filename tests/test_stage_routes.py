"""ResNet.stage_route: the entry every Bottleneck of a stage closes through, planned by shape.

The planner is pure -- module structure, the class-attribute knobs, native.fewrow_enabled() and the library's shape queries, which launch
nothing -- so the whole table is checked here, without a GPU.  tests/test_stage_routes_gpu.py checks that a forward issues what was planned.
A route prints as `step, step xN, ... -> HxW [compact]` (backbone.Route.__str__)."""
import contextlib

import pytest
import torch

from hvrnet_amd import native
from hvrnet_amd.backbone import Bottleneck, ResNet

BF16, F16, SPLIT, F32 = torch.bfloat16, torch.float16, native.SPLIT, torch.float32
DCN = dict(modulated=False, deformable_groups=1, fallback_on_stride=False)


def _net(**kw):
    args = dict(depth=101, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe')
    args.update(kw)
    return ResNet(**args)


_NET = []


def _default():
    if not _NET:
        _NET.append(_net())
    return _NET[0]


def _routes(net, B, H, W, dt):
    out, compact = [], False
    for i in range(len(net.res_layers)):
        out.append(net.stage_route(i, B, H, W, dt, compact))
        (H, W), compact = out[-1].out_hw, out[-1].compact
    return out


def _table(net, B, H, W, dt):
    return [str(r) for r in _routes(net, B, H, W, dt)]


def _fused(hw1, hw2, layer3):
    return ['tail_next(projection), tail_next_live, close_sampled/1 -> %s compact' % hw1,
            'tail_next(projection), tail_next(identity), tail_next_live, conv@compact -> %s compact' % hw2,
            '%s -> %s' % (layer3, hw2)]


def _split(hw0, hw1, hw2):
    return ['downsample+tail_next(identity), tail_next_live, close_sampled/1 -> %s compact' % hw1,
            'downsample+conv, conv x3 -> %s' % hw1, 'downsample+conv, conv x22 -> %s' % hw2]


def _f32(hw0, hw1, hw2):
    return ['downsample+conv, conv x2 -> %s' % hw0, 'downsample+conv, conv x3 -> %s' % hw1, 'downsample+conv, conv x22 -> %s' % hw2]


@pytest.mark.parametrize('B', [1, 15, 60])
def test_routes_of_the_benchmark_map(B):
    """Stage input (B, 152, 252): a 608 x 1008 frame behind the stem."""
    net = _default()
    layer3 = 'tail, tail_next(identity) x21, conv' if B == 60 else 'tail, conv x22'   # (1024, 256) rides from 512 panels up
    for dt in (BF16, F16):
        assert _table(net, B, 152, 252, dt) == _fused('76x126', '38x63', layer3)
    assert _table(net, B, 152, 252, SPLIT) == _split('152x252', '76x126', '38x63')
    assert _table(net, B, 152, 252, F32) == _f32('152x252', '76x126', '38x63')


@pytest.mark.parametrize('shape,sizes', [((2, 53, 75), ('53x75', '27x38', '14x19')), ((1, 50, 74), ('50x74', '25x37', '13x19'))])
def test_routes_of_the_small_test_maps(shape, sizes):
    net = _default()
    for dt in (BF16, F16):
        assert _table(net, *shape, dt) == _fused(sizes[1], sizes[2], 'tail, conv x22')
    assert _table(net, *shape, SPLIT) == _split(*sizes)
    assert _table(net, *shape, F32) == _f32(*sizes)


def test_a_compact_map_under_one_panel_has_no_live_or_sampled_form():
    """(1, 16, 16): the compact map of layer 1 would have 64 pixels, under the 128 of one row panel."""
    net = _default()
    for dt in native.COMPUTE_DTYPES:
        for r in _routes(net, 1, 16, 16, dt):
            assert not r.compact and all(s.kind not in ('tail_next_live', 'close_sampled') and not s.compact for s in r.steps)
    assert _table(net, 1, 16, 16, BF16)[:2] == ['tail_next(projection), tail_next(identity), conv -> 16x16', 'tail, conv x3 -> 8x8']


def test_the_records_behind_the_printed_route():
    net = _default()
    for dt in native.COMPUTE_DTYPES:
        for B in (1, 60):
            for i, r in enumerate(_routes(net, B, 152, 252, dt)):
                assert len(r.steps) == (3, 4, 23)[i]
                for j, s in enumerate(r.steps):
                    assert s.h1_in == (j > 0 and r.steps[j - 1].kind in ('tail_next', 'tail_next_live'))
                    assert s.compact == (j > 0 and r.steps[j - 1].kind == 'tail_next_live')
                    assert s.downsample <= (j == 0) and s.projection <= (j == 0 and not s.downsample)
                    assert (s.stride is not None) == (s.kind == 'close_sampled')
                assert r.compact == (r.steps[-1].compact or r.steps[-1].kind == 'close_sampled')


@pytest.mark.parametrize('how', ['fuse_next_off', 'no_live_store_stages', 'fewrow_split'])
def test_knobs_that_take_the_live_form_away(how, monkeypatch):
    ctx = contextlib.nullcontext()
    if how == 'fuse_next_off':
        monkeypatch.setattr(Bottleneck, 'fuse_next', False)
        want = ['tail, conv, close_sampled/2 -> 76x126 compact', 'tail, conv x3 -> 76x126', 'tail, conv x22 -> 38x63']
    elif how == 'no_live_store_stages':
        monkeypatch.setattr(ResNet, 'live_store_stages', ())
        want = ['tail_next(projection), tail_next(identity), close_sampled/2 -> 76x126 compact',
                'tail_next(projection), tail_next(identity) x2, conv -> 76x126', 'tail, conv x22 -> 38x63']
    else:
        ctx = native.fewrow_split(True)
        want = ['tail_next(projection), tail_next(identity), conv -> 152x252', 'tail_next(projection), tail_next(identity) x2, conv -> 76x126',
                'tail, conv x22 -> 38x63']
    with ctx:
        assert _table(_default(), 1, 152, 252, BF16) == want


def test_fuse_tail_off_closes_projection_blocks_through_convs(monkeypatch):
    monkeypatch.setattr(Bottleneck, 'fuse_tail', False)
    assert _table(_default(), 1, 152, 252, BF16) == [
        'downsample+conv, tail_next_live, close_sampled/1 -> 76x126 compact',
        'downsample+conv, tail_next(identity), tail_next_live, conv@compact -> 38x63 compact', 'downsample+conv, conv x22 -> 38x63']


def test_layer_2_in_compact_stages_closes_through_the_sampled_close(monkeypatch):
    monkeypatch.setattr(ResNet, 'compact_stages', (0, 1))
    got = _table(_default(), 15, 152, 252, BF16)
    assert got == _fused('76x126', '38x63', 'tail, conv x22')[:1] + [
        'tail_next(projection), tail_next(identity), tail_next_live, close_sampled/1 -> 38x63 compact', 'tail, conv x22 -> 38x63']


def _row_panel_closes(net, B, H, W, dt):
    """(stage, block) of every 'conv' close that hvr_conv2d_nhwc runs on the row-panel kernel (hvr_conv2d_path 1)."""
    found, compact = [], False
    for i, r in enumerate(_routes(net, B, H, W, dt)):
        planes = 64 * 2 ** i
        full = (H, W) if compact else ((H - 1) // net.strides[i] + 1, (W - 1) // net.strides[i] + 1)   # the stage's full-resolution map
        for j, s in enumerate(r.steps):
            h, w = r.out_hw if s.compact else full
            if s.kind == 'conv' and native.conv2d_path(B, h, w, planes, 4 * planes, dtype=dt, tile=native.TILE_HINT) == 1:
                found.append((i, j))
        (H, W), compact = r.out_hw, r.compact
    return found


def test_why_layer_2_is_not_in_compact_stages(monkeypatch):
    """The reason behind ResNet.compact_stages = (0,): in a bf16 window (15 frames) layer 2's dense close on its compact map is the only
    closing conv that reaches the row-panel kernel through hvr_conv2d_nhwc, the route the forward-kernel census
    (tests/test_forward_kernels_gpu.py) checks against f64; with layer 2 in compact_stages no conv of the window would take it."""
    assert ResNet.compact_stages == (0,) and ResNet.live_store_stages == (0, 1)
    assert _row_panel_closes(_default(), 15, 152, 252, BF16) == [(1, 3)]
    monkeypatch.setattr(ResNet, 'compact_stages', (0, 1))
    assert _row_panel_closes(_default(), 15, 152, 252, BF16) == []


@pytest.mark.parametrize('how', ['skip_dead_pixels_off', 'pytorch_style', 'every_stage_returned', 'dcn_last_block'])
def test_no_stage_ends_compact_where_its_pixels_are_read(how, monkeypatch):
    if how == 'skip_dead_pixels_off':
        monkeypatch.setattr(ResNet, 'skip_dead_pixels', False)
    net = {'skip_dead_pixels_off': _default, 'pytorch_style': lambda: _net(style='pytorch'), 'every_stage_returned': lambda: _net(out_indices=(0, 1, 2)),
           'dcn_last_block': lambda: _net(dcn=DCN, stage_with_dcn=(True, True, False))}[how]()
    for dt in native.COMPUTE_DTYPES:
        for r in _routes(net, 15, 152, 252, dt):
            assert not r.compact and all(s.kind not in ('tail_next_live', 'close_sampled') and not s.compact for s in r.steps)
    assert [r.out_hw for r in _routes(net, 15, 152, 252, BF16)] == [(152, 252), (76, 126), (38, 63)]


def test_the_tensor_queries_are_the_shape_queries_behind_their_preconditions():
    """CPU tensors fail the device precondition of every *_supported form; the shape forms answer without tensors."""
    h, x, r = torch.zeros(1, 16, 16, 64, dtype=BF16), torch.zeros(1, 16, 16, 64, dtype=BF16), torch.zeros(1, 16, 16, 256, dtype=BF16)
    w3, wt, wn, b = torch.zeros(256, 64, dtype=BF16), torch.zeros(256, 128, dtype=BF16), torch.zeros(64, 256, dtype=BF16), torch.zeros(256)
    assert native.tail_path(1, 16, 16, 64, 256, (16, 16, 64)) and not native.bottleneck_tail_supported(h, x, wt, b, 1)
    assert native.tail_next_path(1, 16, 16, 64, 256, 64, (16, 16, 64)) and not native.bottleneck_tail_next_supported(h, x, None, wt, b, 1, wn, b)
    assert native.tail_next_path(1, 16, 16, 64, 256, 64) and not native.bottleneck_tail_next_supported(h, None, r, w3, b, 1, wn, b)
    assert native.tail_next_live_path(1, 16, 16, 64, 256, 64) and not native.bottleneck_tail_next_live_supported(h, r, w3, b, wn, b, 2)
    assert native.close_sampled_path(1, 16, 16, 64, 256, 16, 16, 1) and not native.bottleneck_close_sampled_supported(h, w3, b, r, 1)
    # no projection form in split half or exact f32, no fused tail in split half; the identity form of tail_next is there in split half
    assert not native.tail_next_path(1, 16, 16, 64, 256, 64, (16, 16, 64), dtype=SPLIT) and native.tail_next_path(1, 16, 16, 64, 256, 64, dtype=SPLIT)
    assert not native.tail_path(1, 16, 16, 64, 256, (16, 16, 64), dtype=SPLIT) and not native.tail_path(1, 16, 16, 64, 256, (16, 16, 64), dtype=F32)
    assert not native.tail_next_path(1, 16, 16, 64, 256, 64, dtype=F32)
