"""GPU tests of the generalized attention block: the core (native.gen_attention: the kernel of csrc/gen_attn.hip in bf16 / half, the torch
composite in all four modes) against the f64 statement of tests/gen_attention_refs.py on the stored operands with its derived bounds, over
a grid of shapes that walks the kernel's tiles; the overflow family; the exact cases; determinism; the reference's golden modules and
Bottlenecks; and a small graphed window with attention blocks in layers 2 and 3."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hvrnet_amd  # noqa: E402
from hvrnet_amd import backbone, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import dcn_refs as D  # noqa: E402
from tests import forward_kernel_refs as F  # noqa: E402
from tests import gen_attention_refs as R  # noqa: E402
from tests.test_gen_attention_refs import BARE, BLOCKS, golden  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': native.SPLIT, 'f32': torch.float32}
# (mode, route): the kernel in its two formats, the composite in all four (split half reaches the core as the f32 form of its values)
RUNS = (('bf16', 'kernel'), ('f16', 'kernel'), ('bf16', 'composite'), ('f16', 'composite'), ('f16x2', 'composite'), ('f32', 'composite'))
QT, KB = native.gen_attn_tiles() if os.path.exists(native.LIB_PATH) else (64, 64)
GRID = R.grid(QT, KB)


def _core_mode(mode):
    return 'f32' if mode == 'f16x2' else mode


def _run(c, mode, route):
    """The core on the device for the stored-format operands c (gen_attention_refs.core_case / block_operands) -> o [B,P,heads,d] f64."""
    dt = DTYPES[_core_mode(mode)]
    B, Mk, heads, d = c['v'].shape

    def dev(a, *shape):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV).to(dt).reshape(*shape).contiguous()

    def f32(a, *shape):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV).reshape(*shape).contiguous()
    o = native.gen_attention(dev(c['q'], B, -1, heads * d), dev(c['k'], B, Mk, heads * d), dev(c['v'], B, Mk, heads * d), heads, d, c['H'], c['W'], c['Hk'],
                             c['Wk'], appr_bias=f32(c['ab'], heads * d), px=dev(c['px'], heads, c['W'], c['Wk'], d), py=dev(c['py'], heads, c['H'], c['Hk'], d),
                             gx=f32(c['gx'], heads, c['W'], c['Wk']), gy=f32(c['gy'], heads, c['H'], c['Hk']), qk=c['qk'], route=route)
    assert o.dtype == dt and tuple(o.shape) == (B, c['H'] * c['W'], heads * d)
    return o


def _vals(o, heads):
    v = o.double().cpu().numpy()
    return v.reshape(v.shape[0], v.shape[1], heads, -1)


def _statement(c, mistake=None):
    return R.core_statement(c['q'], c['k'], c['v'], c['H'], c['W'], c['Hk'], c['Wk'], c['ab'], c['px'], c['py'], c['gx'], c['gy'], c['qk'], mistake)


def _bound(c, r, mode, route):
    return R.core_bound(c['q'], c['k'], c['v'], c['H'], c['W'], c['Hk'], c['Wk'], r, _core_mode(mode), c['ab'], c['px'], c['py'], c['gx'], c['gy'], c['qk'],
                        p_round=None if route == 'kernel' else R.U32, key_block=KB)


def _hold(c, mode, route, what):
    r = _statement(c)
    got = _vals(_run(c, mode, route), c['v'].shape[2])
    bound = _bound(c, r, mode, route)
    err = np.abs(got - r['o'])
    print('%s %s %s: worst |err| / bound = %.3f (|err| max %.3g)' % (what, mode, route, float((err / bound).max()), float(err.max())))
    assert np.isfinite(got).all() and R.outside(got, r['o'], bound) == 0, (what, mode, route, float((err / bound).max()))
    return r, got, bound


# ------------------------------------------------------------------------------------------------ the core
@pytest.mark.parametrize('mode,route', RUNS)
@pytest.mark.parametrize('gi', range(len(GRID)))
def test_core_against_statement(gi, mode, route):
    """All eleven types at one (H, W, s) of the grid; d, heads and B cycle through (16, 32, 64) x (1, 8) x (1, 3) across types and shapes."""
    H, W, s = GRID[gi]
    for i, t in enumerate(R.TYPES):
        d, heads, B = (16, 32, 64)[(i + gi) % 3], (1, 8)[(i + gi // 3) % 2], (1, 3)[(i // 2 + gi) % 2]
        c = R.core_case(B, heads, d, H, W, s, t, mode, 100 * gi + i)
        _hold(c, mode, route, 'type %s d=%d heads=%d B=%d %dx%d/%d' % (t, d, heads, B, H, W, s))


@pytest.mark.parametrize('mode,route', (('bf16', 'kernel'), ('bf16', 'composite')))
def test_core_at_the_real_layer3_shape(mode, route):
    c = R.core_case(1, 2, 32, 38, 63, 2, '1111', mode, 7)
    assert c['Hk'] * c['Wk'] == 608
    _hold(c, mode, route, 'layer 3')


def _overflow_case(mode, peak, seed):
    """Type '1001' on 24 x 24 pixels, s = 1 (576 keys = 9 key blocks of 64 in row order): the y table carries the energies, about +-60 in the
    middle rows, +100 in the key row at one end ('first': row 0, inside the first key block; 'last': row 23, the last block) and -100 at
    the other, whose weights underflow to exactly 0 in f32.  exp(100) overflows f32: without the running maximum the result is inf / inf."""
    c = R.core_case(2, 2, 16, 24, 24, 1, '1001', mode, seed)
    g = np.random.default_rng(seed)
    gy = g.uniform(-60.0, 60.0, c['gy'].shape)
    hi, lo = (0, 23) if peak == 'first' else (23, 0)
    gy[:, :, hi], gy[:, :, lo] = g.uniform(97.0, 100.0, gy[:, :, hi].shape), g.uniform(-103.0, -100.0, gy[:, :, lo].shape)
    c['gy'] = gy.astype(np.float32).astype(np.float64)
    return c


@pytest.mark.parametrize('mode,route', RUNS)
@pytest.mark.parametrize('peak', ('first', 'last'))
def test_overflow_family(peak, mode, route):
    c = _overflow_case(_core_mode(mode), peak, 11)
    r, got, bound = _hold(c, mode, route, 'overflow ' + peak)
    assert np.abs(r['E']).max() > 95.0
    assert R.outside(_statement(c, 'no_max')['o'], r['o'], bound) > 0


@pytest.mark.parametrize('mode,route', RUNS)
def test_exact_cases(mode, route):
    cm = _core_mode(mode)
    # one key: o == v bit for bit, for every type
    for (H, W, s) in ((1, 1, 1), (2, 2, 2), (3, 3, 4)):
        for i, t in enumerate(R.TYPES):
            c = R.core_case(2, (1, 8)[i % 2], (16, 32, 64)[i % 3], H, W, s, t, cm, 300 + i)
            got = _vals(_run(c, mode, route), c['v'].shape[2])
            assert np.array_equal(got, np.broadcast_to(c['v'], got.shape)), (t, H, W, s)
    # v constant over the keys: o equals it within one rounding, whatever the energies
    c = R.core_case(2, 2, 32, 9, 21, 2, '1111', cm, 31, energy_scale=3.0)
    c['v'] = np.broadcast_to(c['v'][:, :1], c['v'].shape).copy()
    got = _vals(_run(c, mode, route), 2)
    want = np.broadcast_to(c['v'][:, :1], got.shape)
    if cm in ('bf16', 'f16'):
        assert (np.abs(got - want) <= R.STORE_REL[cm] * np.abs(want) + R.STORE_ABS[cm]).all()
    else:
        # an f32 map: the f32 chains over the keys are no longer below the format's rounding; the bound with zero spread is all of them
        r = _statement(c)
        bound = _bound(c, r, mode, route)
        assert R.outside(got, want, bound) == 0 and (bound <= (2 * (c['v'].shape[1] + 2 + R.K_ACC) + 2) * R.SECOND * R.U32 * np.abs(want) * 1.001).all()
    # all energies equal (q = 0): o is the mean of v
    c = R.core_case(2, 2, 16, 9, 21, 2, '1000', cm, 32)
    c['q'] = np.zeros_like(c['q'])
    r, got, bound = _hold(c, mode, route, 'uniform')
    assert np.abs(r['o'] - c['v'].mean(1, keepdims=True)).max() < 1e-12


@pytest.mark.parametrize('mode', ('bf16', 'f16'))
def test_two_calls_give_the_same_bits(mode):
    c = R.core_case(3, 8, 32, 17, 35, 2, '1111', mode, 41)
    a, b = _run(c, mode, 'kernel'), _run(c, mode, 'kernel')
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a.float().abs().max()) > 0


def test_refused_calls():
    c = R.core_case(1, 9, 8, 5, 7, 1, '1001', 'bf16', 51)
    with pytest.raises(native.HvrError, match='no kernel'):
        _run(c, 'bf16', 'kernel')
    with pytest.raises(native.HvrError, match='no kernel'):
        _run(R.core_case(1, 2, 16, 5, 7, 1, '1001', 'f32', 52), 'f32', 'kernel')
    _hold(c, 'bf16', None, 'd = 8 by the automatic route (composite)')


# ------------------------------------------------------------------------------------------------ whole modules
def _module(name):
    sd = golden(name)[0]
    m = ops.GeneralizedAttention(**BARE[name])
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval(), sd


def test_golden_modules_on_the_device_in_f32():
    """The reference's five stand-alone modules and two Bottlenecks through this project's modules in f32 mode: the modules within the f32
    block bound of the statement, the Bottlenecks within gen_attention_refs.bottleneck_bound_f32 (derivations there)."""
    for name in sorted(BARE):
        m, sd = _module(name)
        _, x, out, _ = golden(name)
        backbone.set_compute_dtype(m, torch.float32)
        xt = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))).float().to(DEV)
        with torch.no_grad():
            y = m(xt)
            y2 = m.forward_nhwc(backbone.as_nhwc(xt, torch.float32))
        assert torch.equal(y.permute(0, 2, 3, 1), y2)                    # the two layouts agree
        prm = R.block_params(sd, BARE[name])
        r = R.block_statement(x, prm)
        bound = R.block_bound(x, prm, 'f32', r, p_round=R.U32)
        err = np.abs(y2.double().cpu().numpy() - out)
        print('golden %s in f32: worst |err| / bound = %.3f (|err| max %.3g)' % (name, float((err / bound).max()), float(err.max())))
        assert (err <= bound + np.abs(r['y'] - out)).all()
    down = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, stride=2, bias=False), torch.nn.BatchNorm2d(128))
    blocks = dict(f=backbone.Bottleneck(256, 64, gen_attention=BLOCKS['f'][0]),
                  g=backbone.Bottleneck(64, 32, stride=2, downsample=down, gen_attention=BLOCKS['g'][0],
                                        gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))))
    for name, blk in blocks.items():
        sd, x, out, _ = golden(name)
        blk.load_state_dict({k: torch.from_numpy(v).float() if v.dtype == np.float64 and v.ndim else torch.tensor(int(v)) for k, v in sd.items()}, strict=True)
        blk = blk.to(DEV).eval()
        backbone.set_compute_dtype(blk, torch.float32)
        with torch.no_grad():
            y = blk(torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))).float().to(DEV)).permute(0, 2, 3, 1)
        err = float(np.abs(y.double().cpu().numpy() - out).max())
        print('golden %s in f32: max |y - ref| = %.3g of scale %.3g' % (name, err, float(np.abs(out).max())))
        assert tuple(y.shape) == out.shape and err <= R.bottleneck_bound_f32(float(np.abs(out).max()))


# every golden module in every mode; 'd' has 72 channels, which the split-half container (groups of 32 channels) cannot hold
MODULE_RUNS = [(n, m) for n in ('a', 'b', 'c', 'd', 'e', 'fa', 'ga') for m in R.MODES if not (n == 'd' and m == 'f16x2')]


@pytest.mark.parametrize('name,mode', MODULE_RUNS)
def test_modules_in_the_compute_modes(name, mode):
    """A module whose projection weights are values of the mode (the device rounds nothing at pack time but gamma W) on a stored map, against
    the statement with the block bound.  'fa' is the attention block of golden Bottleneck f: d = 16, the kernel route in bf16 / half.
    'd' (72 channels, nine heads of 8) is the zero-padded path: maps and weights padded to the conv entries' channel multiple; so is 'ga',
    the '0111' attention block of golden Bottleneck g on a 32-channel map (two heads of 16)."""
    if name in ('fa', 'ga'):
        full = golden(name[0])[0]
        sd = {k[len('gen_attention_block.'):]: v for k, v in full.items() if k.startswith('gen_attention_block.')}
        C = 64 if name == 'fa' else 32
        cfg = dict(in_dim=C, **BLOCKS[name[0]][0])
        x = R.stored(np.random.default_rng(61).standard_normal((2, 6, 9, C)), mode)
    else:
        sd, cfg = golden(name)[0], BARE[name]
        x = R.stored(golden(name)[1], mode)
    sd = {k: (R.stored(v, mode) if k.endswith('_conv.weight') and not k.startswith('proj') else v) for k, v in sd.items()}
    m = ops.GeneralizedAttention(**cfg)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    backbone.set_compute_dtype(m, DTYPES[mode])
    prm = R.block_params(sd, cfg)
    mult, (H, W), s = (64 if mode in ('bf16', 'f16') else 32), x.shape[1:3], prm['s']
    kernel = native.gen_attn_route(prm['d'], prm['heads'], H, W, (H - 1) // s + 1, (W - 1) // s + 1, DTYPES[_core_mode(mode)],
                                   channels=-(-prm['heads'] * prm['d'] // mult) * mult) == 'kernel'
    assert kernel == (name == 'fa' and mode in ('bf16', 'f16'))
    with torch.no_grad():
        y = m.forward_nhwc(D.to_device_operand(torch.from_numpy(x), mode, DEV))
    r = R.block_statement(x, prm)
    bound = R.block_bound(x, prm, mode, r, p_round=None if kernel else R.U32, key_block=KB)
    err = np.abs(F.values(y).cpu().numpy() - r['y'])
    print('module %s in %s: worst |err| / bound = %.3f (|err| max %.3g, bound max %.3g)' % (name, mode, float((err / bound).max()), float(err.max()), float(bound.max())))
    assert (err <= bound).all() and bound.max() < np.abs(r['y']).max()
    # Link by link the test is sharper than the chained bound (which takes every rounding of q and k against the energies at once): the
    # core on the DEVICE's own projections and tables within the core bound, and the module equal to the chain of public calls
    if mode == 'f16x2':
        return
    xd = D.to_device_operand(torch.from_numpy(x), mode, DEV)
    p, t = m.packed(xd.device), prm['t']
    heads, d, Cq = prm['heads'], prm['d'], prm['heads'] * prm['d']
    assert p['cin'] == -(-x.shape[-1] // mult) * mult and p['cq'] == -(-Cq // mult) * mult and (p['cin'] != x.shape[-1]) == (name == 'd' or (name == 'ga' and mult == 64))
    resid = xd
    if p['cin'] != xd.shape[-1]:
        xd = torch.nn.functional.pad(xd, (0, p['cin'] - xd.shape[-1])).contiguous()
    with torch.no_grad():
        q = native.conv2d_nhwc(xd, p['q']) if (t[0] or t[1]) else None
        k = native.conv2d_nhwc(xd, p['k'], stride=s) if (t[0] or t[2]) else None
        v = native.conv2d_nhwc(xd, p['v'], stride=s)
    tabs = m.position_tables(H, W, xd.device, DTYPES[mode]) if (t[1] or t[3]) else {}
    num = lambda a, *shape: None if a is None else a.double().cpu().numpy().reshape(*shape, -1)[..., :Cq].reshape(*shape, heads, d)   # noqa: E731
    B = x.shape[0]
    Hk, Wk = (H - 1) // s + 1, (W - 1) // s + 1
    one_row = not (t[0] or t[1] or t[3])
    c = dict(q=num(q, B, H * W), k=num(k, B, Hk * Wk), v=num(v, B, Hk * Wk), ab=R.split_heads(prm['ab'], heads) if t[2] else None, qk=t[0],
             H=1 if one_row else H, W=1 if one_row else W, Hk=Hk, Wk=Wk, **{n: (tabs[n].double().cpu().numpy() if n in tabs else None) for n in ('px', 'py', 'gx', 'gy')})
    with torch.no_grad():
        o = native.gen_attention(q, k, v, heads, d, c['H'], c['W'], Hk, Wk, appr_bias=p.get('ab'), px=tabs.get('px'), py=tabs.get('py'), gx=tabs.get('gx'),
                                 gy=tabs.get('gy'), qk=t[0], channels=Cq, route=None)
    rc = _statement(c)
    got = o.double().cpu().numpy()[..., :Cq].reshape(B, -1, heads, d)
    cb = _bound(c, rc, mode, 'kernel' if kernel else 'composite')
    print('module %s in %s, the core on the device\'s projections: worst |err| / bound = %.3f' % (name, mode, float((np.abs(got - rc['o']) / cb).max())))
    assert R.outside(got, rc['o'], cb) == 0
    if not one_row:
        with torch.no_grad():
            assert torch.equal(native.conv2d_nhwc(o.view(B, H, W, -1), p['o'][0], p['o'][1], resid=resid, relu=False), y)


# g is Bottleneck(64, 32): its 3x3 has 32 input channels, which hvr_conv2d_nhwc takes in the f32-grade modes only (Cin % 64 in bf16 / half;
# no ResNet stage is that narrow).  Its attention block runs in bf16 / half as the module 'ga' above.
@pytest.mark.parametrize('name,mode', (('f', 'bf16'), ('f', 'f16'), ('f', 'f16x2'), ('g', 'f16x2')))
def test_golden_bottlenecks_in_the_compute_modes(name, mode):
    """The reference's two Bottlenecks in the native modes, at the link this change adds: the attention block on the DEVICE's own conv2
    output against the statement on those stored values, within the block bound.  (conv1, conv2, conv3 and the context block are the
    links of the Bottlenecks before this one, held by their own tests; f is the kernel route in bf16 / half, g -- '0111', two heads on a
    32-channel map -- the zero-padded composite.)  The whole block runs and stays finite."""
    sd, x, out, _ = golden(name)
    cfg, stride = BLOCKS[name]
    down = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, stride=2, bias=False), torch.nn.BatchNorm2d(128))
    blk = backbone.Bottleneck(256, 64, gen_attention=cfg) if name == 'f' else backbone.Bottleneck(
        64, 32, stride=2, downsample=down, gen_attention=cfg, gcb=dict(ratio=1. / 4., pooling_type='att', fusion_types=('channel_add', 'channel_mul')))
    pre = 'gen_attention_block.'
    sd = {k: (R.stored(v, mode) if k.startswith(pre) and k.endswith('_conv.weight') and 'proj' not in k else v) for k, v in sd.items()}
    blk.load_state_dict({k: torch.from_numpy(v).float() if v.ndim else torch.tensor(int(v)) for k, v in sd.items()}, strict=True)
    blk = blk.to(DEV).eval()
    backbone.set_compute_dtype(blk, DTYPES[mode])
    xd = D.to_device_operand(torch.from_numpy(R.stored(x, mode)), mode, DEV)
    with torch.no_grad():
        h2 = blk._conv2(xd, None, False, None, None)
        y = blk.gen_attention_block.forward_nhwc(h2)
        whole = blk.forward_nhwc(xd)
    hv = F.values(h2).cpu().numpy()
    prm = R.block_params(sd, cfg, pre)
    kernel = name == 'f' and mode in ('bf16', 'f16')
    r = R.block_statement(hv, prm)
    bound = R.block_bound(hv, prm, mode, r, p_round=None if kernel else R.U32, key_block=KB)
    err = np.abs(F.values(y).cpu().numpy() - r['y'])
    print('golden %s in %s, the attention block on the device\'s conv2: worst |err| / bound = %.3f (|err| max %.3g)' % (name, mode, float((err / bound).max()), float(err.max())))
    assert (err <= bound).all()
    wv = F.values(whole).cpu().numpy()
    assert wv.shape == out.shape and np.isfinite(wv).all()


def test_attention_follows_the_dcn_pair():
    """A block with dcn and gen_attention: body() is the attention block on the deformable conv2's output."""
    from tests.test_gcb_gpu import _randomise
    blk = _randomise(backbone.Bottleneck(256, 64, dcn=dict(modulated=True, deformable_groups=1, fallback_on_stride=False),
                                         gen_attention=dict(num_heads=4, kv_stride=2)), 47).to(DEV).eval()
    blk.gen_attention_block.gamma.data.fill_(0.8)
    blk.conv2_offset.weight.data.mul_(0.3)
    for mode in ('bf16', 'f32'):
        backbone.set_compute_dtype(blk, DTYPES[mode])
        x = D.to_device_operand(torch.randn((2, 9, 11, 256), generator=torch.Generator().manual_seed(48)).double(), mode, DEV)
        with torch.no_grad():
            h2 = blk._conv2(x, None, False, None, None)
            p = blk.packed(x.device)
            h1 = native.conv2d_nhwc(x, p['c1'][0], p['c1'][1], relu=True)
            plain = native.conv2d_nhwc(h1, p['c2'][0], p['c2'][1], relu=True, pad=1)
            assert blk.with_dcn and not torch.equal(h2, plain)                 # conv2 is the deformable one
            h = blk.gen_attention_block.forward_nhwc(h2)
            assert torch.equal(blk.body(x), h) and not torch.equal(h, h2)
            assert torch.equal(blk.forward_nhwc(x), native.conv2d_nhwc(h, p['c3'][0], p['c3'][1], resid=x, relu=True))


def _hand_made_body(blk, x):
    p = blk.packed(x.device)
    h = native.conv2d_nhwc(x, p['c1'][0], p['c1'][1], relu=True, stride=blk.conv1_stride)
    h2 = native.conv2d_nhwc(h, p['c2'][0], p['c2'][1], relu=True, stride=blk.conv2_stride, pad=blk.dilation, dil=blk.dilation)
    return h2, blk.gen_attention_block.forward_nhwc(h2)


@pytest.mark.parametrize('mode', R.MODES)
def test_bottleneck_equals_the_hand_made_chain(mode):
    """body() is conv1, conv2 and the attention block by public calls, bit for bit, and the block closes through whatever close its shape
    plans -- the fused ones included, since a close reads nothing of the body but its output."""
    from tests.test_gcb_gpu import _randomise
    layer = _randomise(backbone.make_res_layer(backbone.Bottleneck, 128, 64, 2, stride=2, style='caffe', gen_attention=dict(num_heads=4, kv_stride=2),
                                               gen_attention_blocks=(0, 1)), 43).to(DEV).eval()
    for b in layer:
        b.gen_attention_block.gamma.data.fill_(0.8)
    backbone.set_compute_dtype(layer, DTYPES[mode])
    assert all(b.with_gen_attention and b.gen_attention_block.qk_embed_dim == 16 for b in layer)
    x = D.to_device_operand(torch.randn((2, 13, 17, 128), generator=torch.Generator().manual_seed(44)).double(), mode, DEV)
    with torch.no_grad():
        for blk in layer:
            step = blk.plan_close(x.shape[0], x.shape[1], x.shape[2], DTYPES[mode])
            assert step.kind in ('tail', 'conv'), step
            h2, h = _hand_made_body(blk, x)
            assert torch.equal(blk.body(x), h) and not torch.equal(h2, h)      # the attention block moves conv2's output
            y = blk.forward_nhwc(x)
            assert torch.equal(y, blk.close(x, h, step)) and float(F.values(y).abs().max()) > 0.5
            print('%s: a %s block closes through %s' % (mode, 'projection' if blk.downsample is not None else 'identity', step))
            x = y
    assert tuple(x.shape) == (2, 7, 9, 256)


# ------------------------------------------------------------------------------------------------ a window with attention blocks
T, NPROP = 3, 16
GA = dict(spatial_range=-1, num_heads=8, attention_type='1111', kv_stride=2)
# (placement, frame size): attention in layers 2 and 3; and the standard placement, layer 3 only, at a frame size where layer 2 is
# compacted and feeds layer3.0's attention block through body(compact_in=True)
WINDOWS = {'layers 2-3': (((), (1,), (0, 5)), (60, 90), (64, 96)), 'layer 3 behind a compact layer 2': (((), (), (0, 5)), (120, 180), (128, 192))}


def _window_model(dtype, swa):
    cfg = hvr_config(frame_interval=T // 2, nms_post=NPROP)
    cfg.model.backbone = dict(cfg.model.backbone, depth=50, gen_attention=GA, stage_with_gen_attention=swa)
    cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
    return hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr', depth=50, gen_attention=GA, stage_with_gen_attention=swa), dtype, DEV)


def _eager(model, clip, metas):
    with torch.no_grad():
        c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
        return model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _core_link(m, h, route):
    """The core of a '1111' module m on the device's own projections of the map h (bf16), by `route`, against the statement on those stored
    values -> worst |err| / core bound."""
    p = m.packed(h.device)
    B, H, W, _ = h.shape
    s, heads, d = m.kv_stride, m.num_heads, m.qk_embed_dim
    Hk, Wk = (H - 1) // s + 1, (W - 1) // s + 1
    q, k, v = native.conv2d_nhwc(h, p['q']), native.conv2d_nhwc(h, p['k'], stride=s), native.conv2d_nhwc(h, p['v'], stride=s)
    tabs = m.position_tables(H, W, h.device, h.dtype)
    num = lambda a, n: a.double().cpu().numpy().reshape(B, n, heads, d)   # noqa: E731
    c = dict(q=num(q, H * W), k=num(k, Hk * Wk), v=num(v, Hk * Wk), ab=p['ab'].double().cpu().numpy().reshape(heads, d), qk=True, H=H, W=W, Hk=Hk, Wk=Wk,
             **{n: tabs[n].double().cpu().numpy() for n in ('px', 'py', 'gx', 'gy')})
    o = native.gen_attention(q, k, v, heads, d, H, W, Hk, Wk, appr_bias=p['ab'], px=tabs['px'], py=tabs['py'], gx=tabs['gx'], gy=tabs['gy'], qk=True, route=route)
    rc = _statement(c)
    got = o.double().cpu().numpy().reshape(B, -1, heads, d)
    cb = _bound(c, rc, 'bf16', route)
    assert R.outside(got, rc['o'], cb) == 0
    return float((np.abs(got - rc['o']) / cb).max())


@pytest.mark.parametrize('which', sorted(WINDOWS))
def test_window_eager_and_graph_replay_are_equal_and_the_routes_agree(which):
    from hvrnet_amd.graphs import GraphedClip
    swa, HW, PAD = WINDOWS[which]
    model = _window_model(torch.bfloat16, swa)
    bb = model.backbone
    assert [tuple(j for j, b in enumerate(getattr(bb, n)) if b.with_gen_attention) for n in bb.res_layers] == list(swa)
    r0 = bb.stage_route(0, T, PAD[0] // 4, PAD[1] // 4, torch.bfloat16)
    r1 = bb.stage_route(1, T, *r0.out_hw, torch.bfloat16, r0.compact)
    assert r0.compact and r1.compact == (not swa[1]), (str(r0), str(r1))
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clips = [torch.cat([S.synth_frame(10 * c + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV) for c in range(2)]
    # the first attention block of the net, its input recorded as the window runs
    first_blk = [b for n in bb.res_layers for b in getattr(bb, n) if b.with_gen_attention][0].gen_attention_block
    seen, fwd = [], first_blk.forward_nhwc
    first_blk.forward_nhwc = lambda h, out=None: (seen.append(h.clone()), fwd(h, out))[1]
    with torch.no_grad():
        c4 = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
        del first_blk.forward_nhwc
        ops.GeneralizedAttention.core_route = 'composite'
        try:
            c4c = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
            yc = first_blk.forward_nhwc(seen[0])
        finally:
            ops.GeneralizedAttention.core_route = None
        ya = first_blk.forward_nhwc(seen[0])
        # (the chained block bound below is wide on these weights; the core on the block's own projections is held tightly, by both routes)
        print('window %s, first attention block, the core on the device\'s projections: kernel worst |err| / bound = %.3f, composite %.3f'
              % (which, _core_link(first_blk, seen[0], 'kernel'), _core_link(first_blk, seen[0], 'composite')))
    assert tuple(c4.shape) == (T, 1024, PAD[0] // 16, PAD[1] // 16) and bool(torch.isfinite(c4.float()).all()) and float(c4.float().abs().max()) > 0
    # at the block where the routes part, each is inside the statement's block bound on the block's own input (the kernel's with the bf16
    # rounding of the probabilities, the composite's without), so they lie within the sum of the two bounds of each other
    hv = seen[0].double().cpu().numpy()
    sd = {k: v.detach().double().cpu().numpy() for k, v in first_blk.state_dict().items()}
    sd = {k: (R.stored(v, 'bf16') if k.endswith('_conv.weight') and not k.startswith('proj') else v) for k, v in sd.items()}
    prm = R.block_params(sd, GA)
    r = R.block_statement(hv, prm)
    bk, bc = R.block_bound(hv, prm, 'bf16', r, key_block=KB), R.block_bound(hv, prm, 'bf16', r, p_round=R.U32, key_block=KB)
    ea, ec = np.abs(ya.double().cpu().numpy() - r['y']), np.abs(yc.double().cpu().numpy() - r['y'])
    print('window %s, first attention block: kernel worst |err| / bound = %.3f, composite %.3f' % (which, float((ea / bk).max()), float((ec / bc).max())))
    assert (ea <= bk).all() and (ec <= bc).all() and (np.abs((ya.double() - yc.double()).cpu().numpy()) <= bk + bc).all() and not torch.equal(ya, yc)
    # on the feature map: the two routes of a block differ by the rounding of the probabilities into bf16 (2^-8 relative on weights that sum
    # to one: at most 2 x 2^-8 of a block's output scale, gen_attention_refs 'output'); behind the first attention block at most nine
    # Bottlenecks follow, each of which stores three maps in bf16 (2^-8 relative each) and passes a shift of its input on with a gain of at
    # most one plus its damped residual branch: 9 x 2 x 2^-8 of the map's largest value bounds what the choice of route can move
    scale = float(c4.float().abs().max())
    diff = float((c4.float() - c4c.float()).abs().max())
    print('window %s: |c4(auto) - c4(composite)| max %.3g of scale %.3g (bound %.3g)' % (which, diff, scale, 18 * 2.0 ** -8 * scale))
    assert diff <= 18 * 2.0 ** -8 * scale
    first = [_eager(model, clip, metas) for clip in clips]
    again = [_eager(model, clip, metas) for clip in clips]
    g = GraphedClip(model, clips[0], metas, rescale=True)
    for rep in range(2):
        for clip, want, want2 in zip(clips, first, again):
            got = g.run(clip).result()
            assert len(got) == len(want) == 2
            assert all(_same(a, b) for a, b in zip(want, want2)), 'two eager calls differ'
            assert all(_same(a, b) for a, b in zip(got, want)), 'graph replay differs from the eager window'
            for dets in got[-1]:
                a = np.asarray(dets)
                assert a.ndim == 2 and a.shape[1] == 5 and np.isfinite(a).all()
