"""GPU tests of the Res2Net path: the slice conv (native.res2_conv3x3, both routes) against the f64 statement of tests/res2_refs.py in
all four compute modes with its slice addressing (sentinel maps, NaN neighbours, guard rows), the runs of units that waves walk, the
exact families (equality with round-to-nearest of the statement, kernel == composite bit for bit), the pitched average pool in its
three uses, the first stem conv, the refused shapes, Bottle2necks against the hand-made chain of public native calls with every link
held to its statement, the reference's golden blocks in f32, and a small Res2Net + Res2Layer window eager / graphed."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import res2_refs as R  # noqa: E402

DEV = 'cuda:0'
SPLIT = native.SPLIT
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': SPLIT, 'f32': torch.float32}
NATIVE_MODES = ('bf16', 'f16')          # the modes res2.hip's slice conv has instances for; f32 and split half run the composite route
GUARD_ROWS = 64
SENTINEL = 7777
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_res2net_block.npz')


def _routes(mode):
    return ('kernel', 'composite', None) if mode in NATIVE_MODES else ('composite', None)


def _embed(v, mode, slot, nslots, fill):
    """The Wp-channel values v [B,H,W,Wp] (f64, or None) as slice `slot` of a map of nslots slices whose other channels hold `fill`."""
    if v is None:
        return None
    B, H, W, Wp = v.shape
    full = torch.full((B, H, W, nslots * Wp), fill, dtype=torch.float64, device=v.device)
    full[..., slot * Wp:(slot + 1) * Wp] = v
    return D.to_device_operand(full, mode, DEV)


def _run(c, geom, mode, route, relu=True):
    """native.res2_conv3x3 on true values: x read from slice 2 of a 4-slice map, add from slice 0 of a 3-slice map, both with NaN in every
    other channel (split half stores NaN as its largest magnitude: as far outside any bracket), into slice 1 of a 4-slice map filled with
    the sentinel, guard rows behind it.  -> (stored values f64 [B,OH,OW,Wp] on the device, raw map [rows, 4 Wp] with its guard rows)"""
    B, H, W, width, s, d = geom
    Wp = R.pad_width(width)
    x = _embed(c['x'], mode, 2, 4, float('nan'))
    a = _embed(c['add'], mode, 0, 3, float('nan'))
    OH, OW = R.out_hw(H, W, s)
    M = B * OH * OW
    buf = torch.full((M + GUARD_ROWS, 4 * Wp), SENTINEL, dtype=DTYPES[mode], device=DEV)
    out = buf[:M].view(B, OH, OW, 4 * Wp)
    y = native.res2_conv3x3(x, 2 * Wp, native.Res2Weight(c['w'].float().to(DEV), DTYPES[mode]), c['bias'].float().to(DEV), add=a, add_off=0, out=out,
                            out_off=Wp, stride=s, dil=d, relu=relu, route=route)
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr()
    # the written slice as a map of its own (split half: a 32-channel group is a whole [hi | lo] unit, so a slice is a container too)
    return F.values(out[..., Wp:2 * Wp].contiguous()), buf


def _untouched(buf, M, Wp):
    return bool((buf[M:] == SENTINEL).all()) and bool((buf[:M, :Wp] == SENTINEL).all()) and bool((buf[:M, 2 * Wp:] == SENTINEL).all())


def _hold(got, c, geom, mode, what, relu=True):
    B, H, W, width, s, d = geom
    ref, mag, absxw = R.slice_conv_statement(c['x'], 0, c['w'], c['bias'], c['add'], 0, relu, s, d, mode)
    lo, hi = R.slice_conv_bracket(ref, mag, absxw, width, mode)
    ratio, bad, worst = F.compare(got.to(ref.device), lo, hi, ref)
    print('%s %s %s: worst |got - ref| / bracket = %.3f, %d of %d outside' % (what, geom, mode, ratio, bad, ref.numel()))
    assert float(ref.abs().max()) > 0.5
    assert bad == 0, (what, geom, mode, ratio, bad, worst)
    assert bool((got[..., width:] == 0).all()), 'the pad channels of the written slice are not exact zeros'


# ------------------------------------------------------------------------------------------------ slice conv vs statement
@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('width', (13, 26, 52, 104, 208))
def test_small_map_every_geometry(mode, width):
    """B = 2, 5 x 7 (70 rows at stride 1, 24 at stride 2: a partly filled last unit) over {stride 1, 2} x {dil 1, 2}, with and without the
    add, with and without ReLU, on every route the mode has.  Neighbour slices and guard rows stay as they were."""
    Wp = R.pad_width(width)
    for i, geom in enumerate(g for g in R.SMALL if g[3] == width):
        for with_add in (False, True):
            c = R.real_slice_case(geom, mode, 200 + 10 * width + i, with_add)
            for relu in (True, False):
                for route in _routes(mode):
                    got, buf = _run(c, geom, mode, route, relu)
                    M = buf.shape[0] - GUARD_ROWS
                    assert _untouched(buf, M, Wp), 'a neighbour slice or a guard row was written'
                    _hold(got.cpu(), c, geom, mode, 'route %s add %d relu %d' % (route, with_add, relu), relu)


@pytest.mark.parametrize('mode', F.MODES)
def test_odd_rows(mode):
    """3 x 19 x 23 at Wp = 128 (1 311 rows = 81 units and 15 rows: a multiple of no tile size; two channel blocks), automatic route."""
    geom = R.ODD[0]
    c = R.real_slice_case(geom, mode, 301, True)
    got, buf = _run(c, geom, mode, None)
    assert _untouched(buf, buf.shape[0] - GUARD_ROWS, 128)
    _hold(got.cpu(), c, geom, mode, 'automatic route')
    assert native.res2_conv3x3_supported(3, 19, 23, 128, 1, 1, DTYPES[mode]) == (mode in NATIVE_MODES)


# (B, H, W, width, stride, dil): maps with more units than twice the launch's wave slots, so that a wave runs its loop over pairs of units
# more than once, SOME waves once more than others, the last unit partly filled.  res2.hip, run_res2_conv3x3: units of 16 output pixels,
# nunits = ceil(M / 16); grid = (gx, Wp / NW), NW = 32 / 64 / 64 / 32 output channels per workgroup at Wp = 32 / 64 / 128 / 224,
# gx = min(ceil(nunits / 16), cap), cap = max(1, 256 wpc / (Wp / NW)), wpc = 2 at Wp <= 64 else 1; wave w of workgroup b takes the
# upw = ceil(nunits / (8 gx)) units from (w gx + b) upw on, two per trip of its loop (a last odd one alone).
LOOPED = [(1, 363, 362, 26, 1, 1),       # 131 406 rows = 8 213 units (14 rows in the last) on 4 096 slots
          (1, 725, 723, 52, 2, 1),       # stride 2 -> 363 x 362 rows again, Wp 64
          (1, 181, 182, 104, 1, 2),      # 32 942 rows = 2 059 units (14 rows) on 1 024 slots, two channel blocks, dilation 2
          (1, 97, 97, 208, 1, 1)]        # 9 409 rows = 589 units (1 row) on 288 slots, seven channel blocks


def _trips(geom):
    """(fewest, most) trips of the pair loop among the waves that have a unit at all, and the rows in the last unit, by the rule above."""
    B, H, W, width, s, d = geom
    Wp = R.pad_width(width)
    OH, OW = R.out_hw(H, W, s)
    M = B * OH * OW
    nunits = (M + 15) // 16
    gy = Wp // {32: 32, 64: 64, 128: 64, 224: 32}[Wp]
    cap = max(1, 256 * (2 if Wp <= 64 else 1) // gy)
    gx = min((nunits + 15) // 16, cap)
    upw = (nunits + 8 * gx - 1) // (8 * gx)
    last = nunits - (nunits - 1) // upw * upw           # units of the last wave that has any
    return (last + 1) // 2, (upw + 1) // 2, M % 16


@pytest.mark.parametrize('geom', LOOPED, ids=lambda g: 'x'.join(str(v) for v in g))
def test_waves_that_walk_over_several_units(geom):
    """The loop over pairs of units, in the two modes the kernel has: on real operands every element inside its bracket; on exact operands
    the result equals round-to-nearest of the statement and the composite route bit for bit.  The f64 statements are evaluated on the
    device (a patch matrix of up to 0.6 GB)."""
    lo_trips, hi_trips, tail = _trips(geom)
    assert lo_trips >= 1 and hi_trips >= 2 and hi_trips == lo_trips + 1 and tail != 0, (lo_trips, hi_trips, tail)
    B, H, W, width, s, d = geom
    Wp = R.pad_width(width)
    for mode in NATIVE_MODES:
        c = R.real_slice_case(geom, mode, 400 + width, True, device=DEV)
        got, buf = _run(c, geom, mode, 'kernel')
        assert _untouched(buf, buf.shape[0] - GUARD_ROWS, Wp)
        _hold(got, c, geom, mode, 'kernel')
        c = R.exact_slice_case(geom, mode, 500 + width, True, device=DEV)
        ref, mag, absxw = R.slice_conv_statement(c['x'], 0, c['w'], c['bias'], c['add'], 0, True, s, d, mode)
        F.assert_exact(R.operand(c['x'], c['add'], mode), c['w'], mag, c['q'], mode, ref)
        got, _ = _run(c, geom, mode, 'kernel')
        assert torch.equal(got, F.round_stored(ref, mode)), 'the kernel is not round-to-nearest of the statement on exact operands'
        assert torch.equal(got, _run(c, geom, mode, 'composite')[0]), 'kernel and composite route differ on exact operands'
        del c, ref, mag, absxw, got, buf
        torch.cuda.empty_cache()


@pytest.mark.parametrize('mode', NATIVE_MODES)
def test_exact_families(mode):
    """Exactly summable operands on the small maps: the kernel returns round-to-nearest of the statement and the composite route's bits."""
    for i, geom in enumerate(R.SMALL):
        for with_add in (False, True):
            c = R.exact_slice_case(geom, mode, 600 + i, with_add)
            ref, mag, absxw = R.slice_conv_statement(c['x'], 0, c['w'], c['bias'], c['add'], 0, True, geom[4], geom[5], mode)
            F.assert_exact(R.operand(c['x'], c['add'], mode), c['w'], mag, c['q'], mode, ref)
            got = _run(c, geom, mode, 'kernel')[0].cpu()
            assert torch.equal(got, F.round_stored(ref, mode)), (geom, with_add)
            assert torch.equal(got, _run(c, geom, mode, 'composite')[0].cpu()), (geom, with_add)


# ------------------------------------------------------------------------------------------------ pool, stem
POOLS = [(3, 1, 1, False, True), (3, 2, 1, False, True), (2, 2, 0, True, False), (1, 1, 0, False, True)]


@pytest.mark.parametrize('mode', F.MODES)
def test_pool_three_uses(mode):
    """The 'stage' pool (both strides), the shortcut pool and the copy at 9 x 11 and 10 x 12, from slice 3 of a NaN-filled map into slice 1 of
    a sentinel map.  Allowance: one rounding to the stored format around an f32 evaluation that errs by at most (taps + 1) 2^-24 times
    the window's mean |x| (res2_refs.pool_bracket).  The 1 x 1 copy is bit-equal."""
    for hw in ((9, 11), (10, 12)):
        v = F.store_true(torch.randn((2,) + hw + (32,), generator=torch.Generator().manual_seed(hw[0])), mode)
        x = _embed(v, mode, 3, 4, float('nan'))
        for k, s, p, ce, inc in POOLS:
            ref, mabs, taps = R.pool_statement(v, k, s, p, ce, inc)
            B, OH, OW, _ = ref.shape
            buf = torch.full((B * OH * OW + GUARD_ROWS, 96), SENTINEL, dtype=DTYPES[mode], device=DEV)
            out = buf[:B * OH * OW].view(B, OH, OW, 96)
            native.avgpool_nhwc(x, k, s, p, ce, inc, x_off=96, C=32, out=out, out_off=32)
            torch.cuda.synchronize()
            assert bool((buf[B * OH * OW:] == SENTINEL).all()) and bool((out[..., :32] == SENTINEL).all()) and bool((out[..., 64:] == SENTINEL).all())
            got = F.values(out[..., 32:64].contiguous()).cpu()
            lo, hi = R.pool_bracket(ref, mabs, taps, mode)
            ratio, bad, _ = F.compare(got, lo, hi, ref)
            print('pool k%d s%d %s %s: worst / bracket = %.3f' % (k, s, hw, mode, ratio))
            assert bad == 0, (k, s, hw, mode, ratio, bad)
            if k == 1:
                assert torch.equal(out[..., 32:64], x[..., 96:128])
            fresh = native.avgpool_nhwc(x, k, s, p, ce, inc, x_off=96, C=32)          # out=None: a map of its own
            assert torch.equal(fresh, out[..., 32:64])


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('shape', [(1, 3, 33, 41), (2, 3, 64, 96)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_stem_first_conv(mode, shape):
    """3 -> 32, 3x3 / 2 from the f32 NCHW image against its f64 statement: (27 + 3) 2^-24 sum|x||w| in f32, then the stored rounding; the
    channels behind the 32 results are exact zeros."""
    g = torch.Generator().manual_seed(shape[2])
    img = torch.randn(shape, generator=g) * 50.0
    w, b = torch.randn((32, 3, 3, 3), generator=g) / 27 ** 0.5, torch.randn((32,), generator=g)
    ref, mag = R.stem_first_statement(img, w, b)
    for channels in (32, 64):
        y = native.stem3x3s2_first(img.to(DEV), w.to(DEV), b.to(DEV), DTYPES[mode], channels=channels)
        torch.cuda.synchronize()
        got = F.values(y).cpu()
        assert tuple(got.shape) == tuple(ref.shape[:3]) + (channels,) and bool((got[..., 32:] == 0).all())
        lo, hi = R.stem_first_bracket(ref, mag, mode)
        ratio, bad, _ = F.compare(got[..., :32], lo, hi, ref)
        print('stem first %s %s: worst / bracket = %.3f' % (shape, mode, ratio))
        assert bad == 0 and float(ref.abs().max()) > 10.0, (shape, mode, ratio, bad)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_shapes_and_aliases():
    bf = torch.bfloat16
    x = torch.zeros((2, 5, 7, 256), dtype=bf, device=DEV)
    b = torch.zeros((64,), device=DEV)
    w = torch.zeros((64, 3, 3, 64), device=DEV)
    with pytest.raises(native.HvrError, match='Wp=96'):
        native.res2_conv3x3(torch.zeros((2, 5, 7, 96), dtype=bf, device=DEV), 0, torch.zeros((96, 3, 3, 96), device=DEV), torch.zeros((96,), device=DEV),
                            route='kernel')
    with pytest.raises(native.HvrError, match='stride 3'):
        native.res2_conv3x3(x, 0, w, b, stride=3, route='kernel')
    with pytest.raises(native.HvrError, match='dil=3'):
        native.res2_conv3x3(x, 0, w, b, dil=3, route='kernel')
    with pytest.raises(native.HvrError, match='multiples of 32'):
        native.res2_conv3x3(x, 16, w, b, route='kernel')
    with pytest.raises(native.HvrError, match='outside the map'):
        native.res2_conv3x3(x, 224, w, b, route='kernel')
    with pytest.raises(native.HvrError, match='y aliases x'):
        native.res2_conv3x3(x, 64, w, b, out=x, out_off=64, route='kernel')
    with pytest.raises(native.HvrError, match='y aliases x'):
        native.res2_conv3x3(x, 64, w, b, out=x, out_off=96, route='kernel')      # half a slice further: the channel windows overlap
    with pytest.raises(native.HvrError, match='y aliases add'):
        native.res2_conv3x3(torch.zeros_like(x), 0, w, b, add=x, add_off=64, out=x, out_off=64, route='kernel')
    native.res2_conv3x3(x, 0, w, b, add=x, add_off=64, out=x, out_off=128, route='kernel')      # slices of ONE map that share no channel are fine
    torch.cuda.synchronize()
    for dt in (torch.float32, SPLIT):
        with pytest.raises(native.HvrError, match='bf16 and half'):
            native.res2_conv3x3(torch.zeros((2, 5, 7, 64), dtype=dt, device=DEV), 0, w, b, route='kernel')
    with pytest.raises(native.HvrError, match='k=4'):
        native.avgpool_nhwc(x, 4, 1, 0)
    with pytest.raises(native.HvrError, match='y aliases x'):
        native.avgpool_nhwc(x, 1, 1, 0, x_off=0, C=64, out=x, out_off=64)
    with pytest.raises(native.HvrError, match='ldy=30'):
        native.stem3x3s2_first(torch.zeros((1, 3, 8, 8), device=DEV), torch.zeros((32, 3, 3, 3), device=DEV), torch.zeros((32,), device=DEV), bf, channels=30)


# ------------------------------------------------------------------------------------------------ modules vs the hand-made chain
def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (1.0 / fan) ** 0.5
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_mean.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_var.data = torch.rand(m.bias.shape, generator=g) + 0.5
    return module


def _link(what, mode, got, lo, hi, ref):
    ratio, bad, _ = F.compare(F.values(got), lo, hi, ref)
    print('  %-10s %s: worst / bracket = %.3f' % (what, mode, ratio))
    assert bad == 0, (what, mode, ratio, bad)


def _conv_link(what, mode, got, st, K):
    ref, mag, absxw = st
    _link(what, mode, got, *F.stored_bracket(ref, F.mfma_bound(mag, absxw, K, mode), mode), ref)


def _branch_values(rw, mode, route):
    """The values [Wp,3,3,Wp] of the operand a branch conv reads: the kernel form, or the composite form without its Cin padding -- whose
    every entry must be an exact zero."""
    if route == 'kernel':
        return F.values(rw.kernel(), 'weight')
    dv = F.values(rw.dense(), 'weight')
    assert not bool(dv[..., rw.Wp:].any())
    return dv[..., :rw.Wp]


def _hand_block(blk, x, mode, route=None):
    """The Bottle2neck's forward as public native calls on its packed weights (the branch convs on `route`), each link checked against its
    statement on the operands it received."""
    p = blk.packed(x.device)
    V = F.values
    wp, width, s, dil, nums = blk.wp, blk.width, blk.stride, blk.dilation, blk.nums
    w1, b1 = p['c1']
    P = native.conv2d_nhwc(x, w1, b1, relu=True)
    _conv_link('conv1', mode, P, F.conv_statement(V(x), V(w1, 'weight'), b1, None, True, 1, 0, 1), blk.inplanes)
    assert all(not bool(V(P)[..., i * wp + width:(i + 1) * wp].any()) for i in range(blk.scale)), 'pad channels behind conv1 are not zero'
    B, H, W, _ = P.shape
    OH, OW = R.out_hw(H, W, s)
    Q = torch.full((B, OH, OW, blk.scale * wp), SENTINEL, dtype=P.dtype, device=P.device)
    auto = 'kernel' if mode in NATIVE_MODES and wp in native.RES2_KERNEL_WIDTHS[DTYPES[mode]] else 'composite'
    for i, (rw, b) in enumerate(p['br']):
        prev = blk.stype == 'normal' and i > 0
        native.res2_conv3x3(P, i * wp, rw, b, add=Q if prev else None, add_off=(i - 1) * wp if prev else 0, out=Q, out_off=i * wp, stride=s, dil=dil,
                            relu=True, route=route)
        Pv, Qv = V(P), V(Q[..., :(i + 1) * wp].contiguous())      # (the slices written so far: the rest still holds the sentinel)
        ref, mag, absxw = R.slice_conv_statement(Pv, i * wp, _branch_values(rw, mode, route or auto), b, Qv if prev else None, (i - 1) * wp, True, s, dil, mode)
        _link('branch %d' % i, mode, Q[..., i * wp:(i + 1) * wp].contiguous(), *R.slice_conv_bracket(ref, mag, absxw, width, mode), ref)
    last = P[..., nums * wp:].contiguous()
    k, ps, pp = (3, s, 1) if blk.stype == 'stage' else (1, 1, 0)
    native.avgpool_nhwc(P, k, ps, pp, False, True, x_off=nums * wp, C=wp, out=Q, out_off=nums * wp)
    ref, mabs, taps = R.pool_statement(V(last), k, ps, pp, False, True)
    _link('carried', mode, Q[..., nums * wp:].contiguous(), *R.pool_bracket(ref, mabs, taps, mode), ref)
    ident = x
    if blk.downsample is not None:
        xi = x
        if s > 1:
            xi = native.avgpool_nhwc(x, s, s, 0, True, False)
            ref, mabs, taps = R.pool_statement(V(x), s, s, 0, True, False)
            _link('pool', mode, xi, *R.pool_bracket(ref, mabs, taps, mode), ref)
        wd, bd = p['ds']
        ident = native.conv2d_nhwc(xi, wd, bd, relu=False)
        _conv_link('shortcut', mode, ident, F.conv_statement(V(xi), V(wd, 'weight'), bd, None, False, 1, 0, 1), blk.inplanes)
    w3, b3 = p['c3']
    y = native.conv2d_nhwc(Q, w3, b3, resid=ident, relu=True)
    _conv_link('conv3', mode, y, F.conv_statement(V(Q), V(w3, 'weight'), b3, V(ident), True, 1, 0, 1), width * blk.scale)
    return y


def _act(shape, mode, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).clamp(min=0.0)
    return D.to_device_operand(F.store_true(x, mode), mode, DEV)


BLOCKS = [   # make_res2_layer's (inplanes, planes, stride, dilation), which block of the layer, input [B, H, W, Cin]
    ((64, 64, 1, 1), 0, (2, 10, 12, 64)),         # layer 1's 'stage' block: stride 1, projection without a pool, width 26
    ((256, 128, 2, 1), 0, (2, 9, 11, 256)),       # a stride-2 'stage' block: both pools at stride 2, the shortcut's edge windows, width 52
    ((512, 256, 2, 1), 1, (2, 6, 7, 1024)),       # a 'normal' block of layer 3: the pre-adds, the copy, width 104
    ((1024, 512, 1, 2), 0, (1, 6, 8, 1024)),      # res5's first block: 'stage' at dilation 1 with a 3x3 / 1 pool, width 208
    ((1024, 512, 1, 2), 1, (1, 6, 8, 2048)),      # res5's other blocks: 'normal' at dilation 2
    ((64, 32, 2, 1), 0, (2, 9, 11, 64)),          # the golden block a: width 13
    ((128, 32, 1, 2), 1, (1, 7, 9, 128)),         # the golden block b (as the second block of a layer)
]


@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('case', range(len(BLOCKS)))
def test_bottle2neck_equals_the_hand_made_chain(mode, case):
    (inplanes, planes, stride, dil), which, shape = BLOCKS[case]
    blk = _randomise(backbone.make_res2_layer(backbone.Bottle2neck, inplanes, planes, 2, 26, 4, stride=stride, dilation=dil), 61 + case)[which]
    blk = blk.to(DEV).eval()
    assert (blk.stype, blk.dilation) == (('stage', 1) if which == 0 else ('normal', dil))
    backbone.set_compute_dtype(blk, DTYPES[mode])
    x = _act(shape, mode, 62 + case)
    with torch.no_grad():
        y = blk.forward_nhwc(x)
        want = _hand_block(blk, x, mode)
        assert torch.equal(y, want)
        assert float(F.values(y).abs().max()) > 0.1
        if mode in NATIVE_MODES:
            for route in ('composite', 'kernel'):
                backbone.Bottle2neck.branch_route = route
                try:
                    yr = blk.forward_nhwc(x)
                finally:
                    backbone.Bottle2neck.branch_route = None
                assert torch.equal(yr, _hand_block(blk, x, mode, route=route)), route


def _golden_sd(z, name):
    return {k[len(name) + 1:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith(name + '.') and k.split('.')[-1] not in ('x', 'out', 'out_f32')}


def test_golden_blocks_and_stem_on_the_device_in_f32():
    """The reference's two f64 Bottle2necks and its stem (tests/golden/g22_res2net_block.npz) through this project's modules in f32 mode.
    The bound, from the formats alone (res2_refs.block_bound_f32 / stem_bound_f32 carry the derivation): a block is five chained links
    -- conv1 (K <= 128), three branch convs in a row (K = 117 each), conv3 over K = 52 with the shortcut (K <= 64) -- each erring by at
    most (K + 3) u sum|x||w|, u = 2^-24, with sum|x||w| some tens of the output's scale: 5 x 131 x 6e-8 x 40 = 1.6e-3 -> 2e-3 of the
    output's largest value; the stem is three chained 3x3 convs (K <= 288): 3 x 291 x 6e-8 x 40 = 2.1e-3.  The fixture's own float32
    evaluation lies inside the same bounds (tests/test_res2_refs.py).  A wrong slice map errs by the output's scale itself."""
    z = np.load(GOLDEN)
    layer = backbone.make_res2_layer(backbone.Bottle2neck, 64, 32, 1, 26, 4, stride=2)
    for name, blk in (('a', layer[0]), ('b', backbone.Bottle2neck(128, 32, stype='normal', dilation=2))):
        blk.load_state_dict(_golden_sd(z, name), strict=True)
        blk = blk.to(DEV).eval()
        backbone.set_compute_dtype(blk, torch.float32)
        with torch.no_grad():
            y = blk(torch.from_numpy(z[name + '.x']).float().to(DEV))
        want = torch.from_numpy(z[name + '.out'])
        assert tuple(y.shape) == tuple(want.shape)
        err = float((y.double().cpu() - want).abs().max())
        print('golden block %s in f32: max |y - ref| = %.3g of scale %.3g' % (name, err, float(want.abs().max())))
        assert err <= R.block_bound_f32(float(want.abs().max()))
    net = hvrnet_amd.Res2Net(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    missing = net.load_state_dict(_golden_sd(z, 'stem'), strict=False)
    assert not missing.unexpected_keys and all(k.startswith('layer') for k in missing.missing_keys)
    net = net.to(DEV)
    backbone.set_compute_dtype(net, torch.float32)
    with torch.no_grad():
        y = net._stem(torch.from_numpy(z['stem.x']).float().to(DEV), net.packed(torch.device(DEV)))
    want = torch.from_numpy(z['stem.out']).permute(0, 2, 3, 1)
    assert tuple(y.shape) == tuple(want.shape)
    err = float((y.double().cpu() - want).abs().max())
    print('golden stem in f32: max |y - ref| = %.3g of scale %.3g' % (err, float(want.abs().max())))
    assert err <= R.stem_bound_f32(float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ a Res2Net window
HW, PAD = (120, 150), (128, 160)
T, NPROP = 3, 16


def _window_model(dtype):
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(type='Res2Net', num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='pytorch', norm_eval=True)
    cfg.model.shared_head = dict(type='Res2Layer', depth=101, stage=3, stride=1, dilation=2, style='pytorch', norm_eval=True, external_conv=True)
    return hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', arch='res2net'), dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_res2net_window_eager_twice_and_graph_replay_are_equal():
    from hvrnet_amd.graphs import GraphedClip
    model = _window_model(torch.bfloat16)
    assert type(model.backbone).__name__ == 'Res2Net' and type(model.shared_head).__name__ == 'Res2Layer'
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [torch.cat([S.synth_frame(10 * c + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV) for c in range(2)]
    with torch.no_grad():
        c4 = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
    assert tuple(c4.shape) == (T, 1024, 8, 10) and bool(torch.isfinite(c4.float()).all()) and float(c4.float().abs().max()) > 0
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
            # per class: [n, 5] boxes + score, finite, scores in [0, 1], inside the frame, and x2 - x1 >= -1, y2 - y1 >= -1: the reference's
            # box decode (mmdet/core/bbox/transforms.py delta2bbox) sets x1 = gx - gw / 2 + 1 / 2 and x2 = gx + gw / 2 - 1 / 2 with gw > 0, so a
            # box narrower than one pixel has x2 - x1 = gw - 1 in (-1, 0), and the clip to the frame is monotone
            for dets in got[-1]:
                a = np.asarray(dets)
                assert a.ndim == 2 and a.shape[1] == 5 and np.isfinite(a).all()
                assert (a[:, 4] >= 0).all() and (a[:, 4] <= 1).all() and (a[:, 2] - a[:, 0] >= -1).all() and (a[:, 3] - a[:, 1] >= -1).all()
                assert (a[:, :4] >= 0).all() and (a[:, [0, 2]] <= HW[1]).all() and (a[:, [1, 3]] <= HW[0]).all()
                n_det += len(a)
    assert n_det > 0
