"""Plain float64 statements of the Res2Net pieces -- the 3x3 conv over a channel slice with a pre-add (hvr_res2_conv3x3,
include/hvr_hip.h; native.res2_conv3x3 on either route), the pitched average pool in its three uses (hvr_avgpool_nhwc), the first stem
conv (hvr_stem3x3s2_first) and a whole Bottle2neck -- written from the rule of mmdet/models/backbones/res2net_v1b.py, independently of
the HIP code and of torch's conv / pool dispatch, with the bounds that tests/test_res2_refs.py (CPU) and tests/test_res2_gpu.py (GPU)
hold the kernels to.

The rule of a block (res2net_v1b.py:67-100): out = relu(bn1(conv1(x))), spx = split(out, width); branch i < scale - 1 takes
sp = spx[i] when i == 0 or the block is a 'stage' block, else sp + spx[i] with sp the branch before; sp = relu(bn_i(conv_i(sp)));
the branches are concatenated and the last slice is appended as it is ('normal') or through AvgPool2d(3, stride, padding=1), which
counts its padding and so always divides by 9 ('stage'); conv3 + bn3 + shortcut + ReLU.  The shortcut of make_res2_layer is
AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False) -> 1x1 conv -> BN.

The padded-slice layout.  On the device the `scale` slices live at pitch Wp = width rounded up to 32 in one map of scale * Wp
channels, and the channels [width, Wp) of every slice are exact zeros: conv1's packed weight and bias have zero rows there
(ReLU(0) = 0), the branch weights [Wp][3][3][Wp] zero rows, zero columns and zero bias, conv3's weight zero columns.  The statement
of every sum stays the reference's: a product with an exact zero weight is an exact 0 (finite activations), a zero activation times
any weight too, and adding an exact 0 to a partial sum changes nothing under any rounding rule, truncation included.  So in any
summation order the additions that can round are those that join non-zero terms, at most 9 * width of them behind one accumulator
of a branch conv (split half: three times that, chain() counts them), although the kernel runs K = 9 Wp and the composite route
K = 9 * (Wp padded to the Cin multiple of the mode).  `pad_layout` builds the padded weights from the real ones and the CPU test
holds the padded block equal to the unpadded one; the bracket of a branch conv is forward_kernel_refs.mfma_bound with K = 9 * width
+ E_EPI on the operand s AS DEFINED: s = x's slice, or with an add round_dtype(f32(x) + f32(add)), which `operand` builds bit for bit
((x.float() + a.float()).to(dtype) in torch).  No bound contains a value measured on a device.

`mistake=` states a plausible mistake exactly (MISTAKES); the CPU tests show each outside the bound on real operands and unequal on
exact ones.
"""
import math

import torch

from tests import forward_kernel_refs as F

U = F.U
WIDTHS = {26: 32, 52: 64, 104: 128, 208: 224}                  # the four stages' slice widths -> Wp
MISTAKES = ('add_same_slice', 'add_in_stage', 'pool_in_normal', 'pool_valid_count', 'shortcut_floor', 'first_dilated', 'pad_nonzero')
# (B, H, W, width, stride, dil): the geometries of tests/test_res2_gpu.py
SMALL = [(2, 5, 7, width, s, d) for width in (13, 26, 52, 104, 208) for s in (1, 2) for d in (1, 2)]
ODD = [(3, 19, 23, 104, 1, 1)]                                  # 1 311 rows at Wp = 128: a multiple of no tile size


def pad_width(width):
    return (width + 31) // 32 * 32


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ------------------------------------------------------------------------------------------------ the slice conv
def operand(xs, adds, mode):
    """The operand the conv multiplies (f64 values): the slice, or round_dtype(f32(x) + f32(add)).  The f64 sum of two stored values
    rounded to f32 IS their f32 sum (both are f32 numbers); then one rounding into the operand format."""
    if adds is None:
        return xs.double()
    s32 = (xs.double() + adds.double()).float()
    return s32.double() if mode == 'f32' else F.round_stored(s32.double(), mode)


def slice_conv_statement(x, x_off, w, bias, add=None, add_off=0, relu=True, stride=1, dil=1, mode='bf16', mistake=None):
    """x [B,H,W,Cx], add [B,H,W,Ca] (stored values, any real dtype), w [Wp,3,3,Wp], bias [Wp] -> (ref, mag, sum|s||w|), f64 [B,OH,OW,Wp]:
    the conv of the Wp channels from x_off on (+ add's from add_off on), pad == dil.  Channels outside the slices are never touched, so
    they may hold NaN."""
    Wp = w.shape[0]
    assert tuple(w.shape) == (Wp, 3, 3, Wp)
    s = operand(x[..., x_off:x_off + Wp], None if add is None else add[..., add_off:add_off + Wp], mode)
    return F.conv_statement(s, w, bias, None, relu, stride, dil, dil, mistake if mistake in ('tap_border', 'dil1') else None)


def slice_conv_bound(mag, absxw, width, mode):
    """Bound on the f32 value before the store: chain 9 * width + E_EPI (module docstring)."""
    return F.mfma_bound(mag, absxw, 9 * width, mode)


def slice_conv_bracket(ref, mag, absxw, width, mode):
    return F.stored_bracket(ref, slice_conv_bound(mag, absxw, width, mode), mode)


def real_slice_case(geom, mode, seed, with_add, device='cpu'):
    """Real-statistics operands for one slice conv: x and add after a ReLU, a [Wp,3,3,Wp] weight whose rows and columns from `width` on are
    zero, a bias with zeros there.  x, add carry ONLY the Wp slice channels, pad channels zero (the callers embed them in wider maps)."""
    B, H, W, width, s, d = geom
    Wp = pad_width(width)
    x, w = F.real_operands((B, H, W, Wp), (Wp, 3, 3, Wp), mode, seed, device=device)
    w = w * math.sqrt(Wp / width)
    w = F.store_true(w.float().cpu(), mode, 'weight').to(device)
    g = torch.Generator().manual_seed(seed + 7)
    bias = (torch.randn((Wp,), generator=g) * 0.3).double().to(device)
    a = F.store_true(torch.randn((B, H, W, Wp), generator=g).clamp(min=0.0), mode, 'act').to(device) if with_add else None
    x[..., width:] = 0
    w[width:] = 0
    w[..., width:] = 0
    bias[width:] = 0
    if a is not None:
        a[..., width:] = 0
    return dict(x=x, w=w, bias=bias, add=a)


def exact_slice_case(geom, mode, seed, with_add, device='cpu'):
    """Exact-sum operands (forward_kernel_refs.exact_case, 'plain': integers of at most four bits x 2^-4): x + add is exact in every
    format too (|sum| <= 30 quanta), every partial sum an f32 number in any order.  -> dict(x, w, bias, add, q)"""
    B, H, W, width, s, d = geom
    Wp = pad_width(width)
    c = F.exact_case((B, H, W, Wp), (Wp, 3, 3, Wp), mode, seed, device=device)
    x, w, bias = c['a'], c['w'], c['bias']
    a = F._ints((B, H, W, Wp), -15, 15, c['g']) * c['q'] if with_add else None
    x[..., width:] = 0
    w[width:] = 0
    w[..., width:] = 0
    bias[width:] = 0
    if a is not None:
        a[..., width:] = 0
    return dict(x=x, w=w, bias=bias, add=a, q=c['q'])


# ------------------------------------------------------------------------------------------------ the average pool
def pool_out(n, k, stride, pad, ceil_mode):
    """torch.nn.AvgPool2d's output size along one axis: ceil instead of floor, and the last window must start inside the map or its
    left padding."""
    span = n + 2 * pad - k
    o = (-(-span // stride) if ceil_mode else span // stride) + 1
    if ceil_mode and (o - 1) * stride >= n + pad:
        o -= 1
    return o


def pool_statement(x, k, stride=1, pad=0, ceil_mode=False, count_include_pad=True, mistake=None):
    """x [B,H,W,C] -> (ref, mean|x| of the window, taps) f64 [B,OH,OW,C] by index arithmetic.  The divisor: with count_include_pad the
    window clipped to the PADDED map (so 9 everywhere for k 3, pad 1, floor), else the number of elements inside the map.
    Mistakes: 'pool_valid_count' divides by the elements inside the map although the padding counts; 'shortcut_floor' sizes the output
    with floor although ceil is asked (the windows of the last row / column are dropped: they read as zero)."""
    x = x.double()
    B, H, W, C = x.shape
    if mistake == 'pool_valid_count':
        count_include_pad = False
    OH, OW = pool_out(H, k, stride, pad, ceil_mode), pool_out(W, k, stride, pad, ceil_mode)
    ref = torch.zeros((B, OH, OW, C), dtype=torch.float64, device=x.device)
    mabs = torch.zeros_like(ref)
    for oy in range(OH):
        for ox in range(OW):
            h0, w0 = oy * stride - pad, ox * stride - pad
            h1, w1 = min(h0 + k, H + pad), min(w0 + k, W + pad)
            full = (h1 - h0) * (w1 - w0)
            h0, w0, h1, w1 = max(h0, 0), max(w0, 0), min(h1, H), min(w1, W)
            div = full if count_include_pad else (h1 - h0) * (w1 - w0)
            win = x[:, h0:h1, w0:w1, :]
            ref[:, oy, ox] = win.sum((1, 2)) / div
            mabs[:, oy, ox] = win.abs().sum((1, 2)) / div
    if mistake == 'shortcut_floor' and ceil_mode:
        fh, fw = pool_out(H, k, stride, pad, False), pool_out(W, k, stride, pad, False)
        ref[:, fh:], mabs[:, fh:] = 0.0, 0.0
        ref[:, :, fw:], mabs[:, :, fw:] = 0.0, 0.0
    return ref, mabs, k * k


def pool_bracket(ref, mabs, taps, mode):
    """One rounding to the stored format around an f32 evaluation that errs by at most (taps + 1) u mean|x|: taps - 1 additions and the
    multiplication by the rounded reciprocal (two roundings), each relative to a partial sum of at most sum|x|."""
    return F.stored_bracket(ref, F.SECOND * (taps + 1) * U * mabs, mode)


# ------------------------------------------------------------------------------------------------ the first stem conv
def stem_first_statement(img, w, bias):
    """img [B,3,H,W], w [32,3,3,3] as [n,ky,kx,c], bias [32] -> (ref, mag) f64 [B,OH,OW,32]: 3x3, stride 2, pad 1, + bias, ReLU."""
    x = img.double().permute(0, 2, 3, 1)
    ref, mag, _ = F.conv_statement(x, w.double(), bias.double(), None, True, 2, 1, 1)
    return ref, mag


def stem_first_bracket(ref, mag, mode):
    """f32 FMAs: (27 + 3) u sum|x||w| (27 fused multiply-adds behind the bias, the epilogue's allowance), then the stored rounding."""
    return F.stored_bracket(ref, F.SECOND * (27 + 3) * U * mag, mode)


# ------------------------------------------------------------------------------------------------ a Bottle2neck as a chain of statements
def fold(sd, conv, bn, eps=1e-5):
    """(w [Cout,KH,KW,Cin], bias) f64 of a conv with its eval-mode BatchNorm folded in, from a state dict of f64 tensors."""
    w = sd[conv + '.weight'].double()
    scale = sd[bn + '.weight'].double() / torch.sqrt(sd[bn + '.running_var'].double() + eps)
    bias = sd[bn + '.bias'].double() - sd[bn + '.running_mean'].double() * scale
    return (w * scale[:, None, None, None]).permute(0, 2, 3, 1).contiguous(), bias


def fold_block(sd, nums=3, downsample=False):
    p = dict(c1=fold(sd, 'conv1', 'bn1'), br=[fold(sd, 'convs.%d' % i, 'bns.%d' % i) for i in range(nums)], c3=fold(sd, 'conv3', 'bn3'))
    if downsample:
        p['ds'] = fold(sd, 'downsample.1', 'downsample.2')
    return p


def pad_layout(p, width, scale, mistake=None):
    """The padded-slice form of folded weights p (module docstring): slices at pitch Wp, exact zeros in the pad rows / columns / biases.
    'pad_nonzero': the pad rows of conv1 get a bias of 1/2 and the pad columns of the branch weights and of conv3 the value 1/64, as
    a packer that fills the padding with something else than zero would leave them."""
    wp = pad_width(width)
    junk_b, junk_w = (0.5, 2.0 ** -6) if mistake == 'pad_nonzero' else (0.0, 0.0)

    def scatter(t, dim, fill):
        shape = list(t.shape)
        shape[dim] = scale * wp
        out = torch.full(shape, fill, dtype=torch.float64)
        for i in range(scale):
            out.narrow(dim, i * wp, width).copy_(t.narrow(dim, i * width, width))
        return out

    q = dict(c1=(scatter(p['c1'][0], 0, 0.0), scatter(p['c1'][1], 0, junk_b)), br=[], c3=(scatter(p['c3'][0], 3, junk_w), p['c3'][1]))
    for w, b in p['br']:
        wpad = torch.zeros((wp, 3, 3, wp), dtype=torch.float64)
        wpad[:width, :, :, width:] = junk_w
        wpad[:width, :, :, :width] = w
        bpad = torch.zeros((wp,), dtype=torch.float64)
        bpad[:width] = b
        q['br'].append((wpad, bpad))
    if 'ds' in p:
        q['ds'] = p['ds']
    return q


def block_statement(x, p, width, scale, stype, stride=1, dil=1, mistake=None):
    """A Bottle2neck in f64 over FOLDED weights p (fold_block; or pad_layout's with `width` = Wp): x [B,H,W,Cin] -> [B,OH,OW,4 planes].
    Mistakes: 'add_same_slice' the add of branch i > 0 read at slice i of the output map instead of i - 1 (the slice being written, which a
    fresh zero-filled map holds as zeros: no add at all); 'add_in_stage' the add applied in a 'stage' block; 'pool_in_normal' the carried
    slice of a 'normal' block pooled 3x3; 'pool_valid_count' / 'shortcut_floor' (pool_statement) in the 'stage' pool / the shortcut
    pool; 'first_dilated' a 'stage' block run at dilation 2."""
    assert mistake is None or mistake in MISTAKES, mistake
    nums = scale - 1
    if mistake == 'first_dilated' and stype == 'stage':
        dil = 2
    P = F.conv_statement(x, p['c1'][0], p['c1'][1], None, True, 1, 0, 1)[0]
    outs = []
    for i, (w, b) in enumerate(p['br']):
        sp = P[..., i * width:(i + 1) * width]
        with_add = i > 0 and (stype == 'normal' or mistake == 'add_in_stage') and mistake != 'add_same_slice'
        if with_add:
            sp = sp + outs[-1]
        outs.append(F.conv_statement(sp, w, b, None, True, stride, dil, dil)[0])
    last = P[..., nums * width:(nums + 1) * width]
    if stype == 'stage' or mistake == 'pool_in_normal':
        last = pool_statement(last, 3, stride, 1, False, True, mistake if mistake == 'pool_valid_count' else None)[0]
    Q = torch.cat(outs + [last], 3)
    idt = x.double()
    if 'ds' in p:
        if stride > 1:
            idt = pool_statement(idt, stride, stride, 0, True, False, mistake if mistake == 'shortcut_floor' else None)[0]
        idt = F.conv_statement(idt, p['ds'][0], p['ds'][1], None, False, 1, 0, 1)[0]
    return F.conv_statement(Q, p['c3'][0], p['c3'][1], idt, True, 1, 0, 1)[0]


def block_bound_f32(scale_of_output):
    """Bound on |device f32 block - f64 fixture| from the formats alone, for the golden blocks (width 13, Cin <= 128): five chained links
    -- conv1 (K = Cin <= 128), three branch convs in a row (K = 9 x 13 = 117 each; in a 'normal' block each feeds the next), conv3 over
    K = 52 with the shortcut (pool + 1x1 over K <= 64) -- each erring by at most (K + 3) u sum|x||w| with u = 2^-24; the f32 rounding of
    the parameters and of the folded weights adds u per factor.  sum|x||w| of a link is some tens of its output's scale (weights
    N(0, 1/K), BatchNorm gains of 0.5 .. 1.5 over sqrt(0.5 .. 1.5)), and an error made in one link passes through the gains of the
    links behind it, each of which is of order one: 5 links x 131 x 6e-8 x 40 = 1.6e-3 -> 2e-3 of the output's largest value.  (A wrong
    slice map errs by the scale itself.)"""
    return 2e-3 * scale_of_output


def stem_bound_f32(scale_of_output):
    """The same for the stem (three chained 3x3 convs, K = 27, 288, 288, then a max pool that selects): 3 x 291 x 6e-8 x 40 = 2.1e-3."""
    return 2.1e-3 * scale_of_output
