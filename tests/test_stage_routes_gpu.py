"""A ResNet forward issues what ResNet.stage_route planned: the closing entries per stage, recorded by wrapping native.* by name
(as tests/test_live_store_gpu.py: _Calls), against the planner's records.  tests/test_stage_routes.py checks the plan itself, on the CPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native  # noqa: E402

DEV = 'cuda:0'
MODES = [torch.bfloat16, torch.float16, native.SPLIT, torch.float32]
MODE_IDS = ['bf16', 'half', 'split_half', 'f32']


def _net():
    from hvrnet_amd import synthetic as S
    from hvrnet_amd.backbone import ResNet
    g = torch.Generator().manual_seed(7)   # seeded weights with live residual branches (as tests/test_dead_pixels_gpu.py: _backbone_state)
    sd = {'conv1.weight': S._conv(g, 64, 3, 7)}
    S._bn(g, sd, 'bn1', 64)
    inplanes = 64
    for i, nb in enumerate((3, 4, 6)):
        S._res_layer(g, sd, 'layer%d' % (i + 1), inplanes, 64 * 2 ** i, nb)
        inplanes = 64 * 2 ** i * 4
    net = ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe', zero_init_residual=False)
    net.load_state_dict(sd)
    return net.to(DEV)


class _Closes(object):
    """The closing entries in issue order, as (Cout, entry, detail): the fused Bottleneck entries, and from conv2d_nhwc the 1x1 convs with a
    residual ('conv', output map) and the projection shortcuts ('downsample': 1x1 without ReLU)."""

    def __init__(self, monkeypatch):
        self.seq = []
        real = {n: getattr(native, n) for n in ('bottleneck_tail', 'bottleneck_tail_next', 'bottleneck_tail_next_live', 'bottleneck_close_sampled',
                                                'conv2d_nhwc')}

        def tail(h, x, w, *a, **k):
            self.seq.append((w.shape[0], 'tail'))
            return real['bottleneck_tail'](h, x, w, *a, **k)

        def tail_next(h, x, resid, w, *a, **k):
            self.seq.append((w.shape[0], 'tail_next', 'projection' if x is not None else 'identity'))
            return real['bottleneck_tail_next'](h, x, resid, w, *a, **k)

        def live(h, resid, w, *a, **k):
            self.seq.append((w.shape[0], 'tail_next_live'))
            return real['bottleneck_tail_next_live'](h, resid, w, *a, **k)

        def sampled(h, w, bias, resid, stride=2, relu=True, out=None):
            self.seq.append((w.shape[0], 'close_sampled', stride))
            return real['bottleneck_close_sampled'](h, w, bias, resid, stride=stride, relu=relu, out=out)

        def conv(x, w, bias=None, resid=None, relu=False, *a, **k):
            y = real['conv2d_nhwc'](x, w, bias, resid, relu, *a, **k)
            if w.shape[1] == 1 and resid is not None:
                self.seq.append((w.shape[0], 'conv', tuple(y.shape[1:3])))
            elif w.shape[1] == 1 and not relu:
                self.seq.append((w.shape[0], 'downsample'))
            return y
        for n, f in (('bottleneck_tail', tail), ('bottleneck_tail_next', tail_next), ('bottleneck_tail_next_live', live),
                     ('bottleneck_close_sampled', sampled), ('conv2d_nhwc', conv)):
            monkeypatch.setattr(native, n, f)


def _planned(route, Cout, full_hw):
    """The calls a Route stands for, in the form _Closes records them."""
    seq = []
    for s in route.steps:
        if s.downsample:
            seq.append((Cout, 'downsample'))
        detail = {'tail_next': ('projection' if s.projection else 'identity',), 'close_sampled': (s.stride,),
                  'conv': (route.out_hw if s.compact else full_hw,)}.get(s.kind, ())
        seq.append((Cout, s.kind) + detail)
    return seq


@pytest.mark.parametrize('dt', MODES, ids=MODE_IDS)
def test_a_forward_issues_the_planned_route(dt, monkeypatch):
    """2 x 3 x 212 x 300: stage maps 53x75 -> 27x38 -> 14x19."""
    from hvrnet_amd import synthetic as S
    from hvrnet_amd.backbone import set_compute_dtype
    net = set_compute_dtype(_net(), dt)
    x = torch.cat([S.synth_frame(i, img_hw=(212, 300), pad_hw=(212, 300)) for i in range(2)]).to(DEV)
    calls = _Closes(monkeypatch)
    with torch.no_grad():
        y = net(x)[0]
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 1024, 14, 19)
    want, (H, W), compact = [], (53, 75), False
    for i in range(3):
        route = net.stage_route(i, 2, H, W, dt, compact)
        full = (H, W) if compact else ((H - 1) // net.strides[i] + 1, (W - 1) // net.strides[i] + 1)
        want += _planned(route, 256 * 2 ** i, full)
        (H, W), compact = route.out_hw, route.compact
    print('\n'.join('%s: %s' % (native.DTYPE_NAMES[dt], c) for c in calls.seq))
    assert calls.seq == want
    if dt in (torch.bfloat16, torch.float16):   # the forms are there to be planned: this map is large enough for each of them
        assert {(256, 'tail_next_live'), (256, 'close_sampled', 1), (512, 'tail_next_live'), (512, 'conv', (14, 19))} <= set(calls.seq)
