"""Plain float64 statements of the BACKWARD of train_ops.ConvFunction and train_ops.LinearFunction -- the compositions of
hvr_relu_bwd(_t), hvr_im2col_t / hvr_transpose_pad, hvr_gemm, hvr_gemm_splitk(_batched), hvr_conv2d_nhwc on rotated weights,
hvr_unpack_conv_wgrad and hvr_colsum -- written by index arithmetic, independently of the HIP code and of torch's conv and autograd,
with the error bounds that tests/test_backward_refs.py (CPU) and tests/test_backward_gpu.py (GPU) hold them to.

Operands enter as STORED values (forward_kernel_refs.values): x is the tensor given to the Function, w_eff the packed operand
[Cout][KH][KW][Cin] = RN(w * s) (native.pack_conv_weight; linear: native.cast(w, dtype)), y the stored output of the Function's own
forward -- the ReLU gate is defined on the stored y, so nothing is ambiguous near zero.

    dz = RN(dy -> compute dtype) where y > 0, else 0            exact: the residual gradient IS dz (torch.equal)
    dx[b, oy - pad + ky dil, ox - pad + kx dil, c] += dz[b, oy, ox, o] w_eff[o, ky, kx, c]          K = KH KW Cout terms
         (a strided 1x1 lands on the pixels (s oy, s ox) of x; every other pixel is exactly 0)
    dw[o, c, ky, kx] = s[o] sum_p dz[p, o] patch[p, ky, kx, c]  parameter layout, f32 result, K = P = B OH OW terms
    dt[o] = sum_p dz[p, o]
    linear: dx = dz wc, dw = dz^T x, db = column sums of dz

Error model: that of tests/forward_kernel_refs.py (f32 chain: u per added term, 16-bit operands: 2u; E_EPI = 3 operations behind the
accumulator; all x SECOND).  Nothing here is measured on a device.
  dX        stored_bracket(ref, mfma_bound(mag, mag, K, mode), mode): one rounding of the f32 accumulator to the compute dtype.
  dW (f32)  |s[o]| mfma_bound(mag, mag, P, mode).  The any-order clause of the forward model covers the split-K slices and their
            reduce (the longest chain behind one element is at most P); E_EPI = 3 covers the reduce's last addition, the
            multiplication by s and the addition into a gradient buffer.  Accumulating into an existing gradient g0 adds
            SECOND u (|g0| + |ref|): the one rounding of g0 + dw.
  db / dt   train_kernel_refs.colsum_bound of the stored dz (the chain of hvr_colsum).
  f32 mode  the same statements under the f32 chain (u per term, one rounding per product).

MISTAKES: plausible mistakes of the composition, each stated exactly (`mistake=`); the CPU tests show every one outside a bracket or
bound on real-statistics operands, or unequal on the exact-sum operands (exact_case below: integers times a quantum, integer dy, s a
power of two, mag <= 2^24 q^2, so dX must be RN(statement) bit for bit and dW exactly s * sum).
"""
import math

import torch

from tests import forward_kernel_refs as R
from tests import train_kernel_refs as K

U = R.U
SECOND = R.SECOND

MISTAKES = ('taps_not_reversed', 'dx_pad_forward', 'dx_dil1', 'mask_from_dy', 'mask_ge', 'dy_unrounded', 'wgrad_no_scale',
            'wgrad_scale_by_cin', 'wgrad_taps_swapped', 'wgrad_dil1', 'pad_rows_live', 'wgrad_last_slice_dropped',
            'stride_scatter_offset', 'accumulate_overwrites', 'dr_unmasked', 'linear_dw_transposed', 'db_row_sums')

# name -> ((B, H, W, Cin, Cout, k, stride, pad, dil), relu, residual, out_f32 (f32 dy, trainable shift)); each the smallest that reaches its
# edge; every ReLU case has a residual, whose gradient shows dz itself
CONV_CASES = {
    'k3_res': ((2, 13, 18, 64, 96, 3, 1, 1, 1), True, True, False),        # P = 468 -> ldp 512; Cout no multiple of 64
    'k3_dil2': ((1, 9, 14, 128, 72, 3, 1, 2, 2), True, True, False),      # dilation 2, Cout = 72
    'k3_pad0': ((2, 7, 9, 72, 136, 3, 1, 0, 1), True, True, False),       # pad != dil (K - 1) / 2: dX's conv pads by 2 ...
    'k3_pad2': ((2, 7, 9, 72, 136, 3, 1, 2, 1), True, True, False),       # ... and by 0
    'k1': ((2, 13, 18, 256, 64, 1, 1, 0, 1), True, True, False),          # 1x1: ldn = Cout
    'k1_s2': ((2, 13, 19, 128, 256, 1, 2, 0, 1), True, True, False),      # strided 1x1, odd H and W: 7 x 10, dX zero off the lattice
    'k1_f32_12': ((1, 6, 8, 128, 12, 1, 1, 0, 1), False, False, True),     # f32 dy rounded once, dt; Cout % 8: the relu_bwd / transpose_pad route
    'k1_f32_48': ((1, 6, 8, 128, 48, 1, 1, 0, 1), False, False, True),
    'k3_long': ((3, 38, 63, 64, 64, 3, 1, 1, 1), True, True, False),      # P = 7182 -> ldp 7232: dW in K slices, the last one ragged
    # the two pad != dil (K - 1) / 2 cases at the nearest Cin the conv kernels take (Cin = 72 is refused: no multiple of the K-step)
    'k3_pad0_c64': ((2, 7, 9, 64, 136, 3, 1, 0, 1), True, True, False),
    'k3_pad2_c64': ((2, 7, 9, 64, 136, 3, 1, 2, 1), True, True, False),
}
REFUSED_CONV_CASES = ('k3_pad0', 'k3_pad2')      # Cin = 72: hvr_conv2d_nhwc refuses (Cin % K-step); the GPU test asserts the refusal

# name -> (M, K, N, relu, resid, bias, out_f32)
LINEAR_CASES = {
    'm37': (37, 128, 72, True, True, True, False),             # M < 64
    'n124': (300, 256, 124, True, False, True, False),         # N % 8: relu_bwd + transpose_pad, not relu_bwd_t
    'logits': (300, 1024, 40, False, False, True, True),       # the fused logits layer, f32 output and f32 dy
    'square': (129, 1024, 1024, True, False, True, False),
}


def out_hw(H, W, k, stride, pad, dil):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def kstep(mode):
    return 32 if mode == 'f32' else 64


def _dz(dy, y, relu, mode, mistake):
    """(dz, dr): the gated, once-rounded upstream gradient and what the residual receives."""
    d = dy.double()
    if mode in ('bf16', 'f16') and mistake != 'dy_unrounded':
        d = dy.float().to(R.STORE[mode]).double()             # RN of an f32 dy to the compute dtype (a no-op on a 16-bit dy)
    if not relu:
        return d, d
    if mistake == 'mask_from_dy':
        gate = dy.double() > 0
    elif mistake == 'mask_ge':
        gate = y.double() >= 0
    else:
        gate = y.double() > 0
    dz = d * gate
    return dz, (d if mistake == 'dr_unmasked' else dz)


def _dx_scatter(dz, w, Hs, Ws, pad, dil, mistake):
    """dz [B, OH, OW, Cout], w [Cout, KH, KW, Cin] -> (dx, sum|dz||w|) [B, Hs, Ws, Cin], tap by tap:
    dx[b, oy + off_y, ox + off_x, :] += dz[b, oy, ox, :] w[:, ky, kx, :] with off = -pad + k dil (clipped to the map)."""
    B, OH, OW, Cout = dz.shape
    _, KH, KW, Cin = w.shape
    dx = torch.zeros((B, Hs, Ws, Cin), dtype=torch.float64, device=dz.device)
    ab = torch.zeros_like(dx)
    dz2 = dz.reshape(-1, Cout)
    # 'dx_pad_forward': the dX conv run with the forward's pad instead of dil (K - 1) - pad: every tap lands 2 pad - dil (K - 1) further
    sy = 2 * pad - dil * (KH - 1) if mistake == 'dx_pad_forward' else 0
    sx = 2 * pad - dil * (KW - 1) if mistake == 'dx_pad_forward' else 0
    for ky in range(KH):
        for kx in range(KW):
            wy, wx = (KH - 1 - ky, KW - 1 - kx) if mistake == 'taps_not_reversed' else (ky, kx)
            oy_, ox_ = -pad + ky * dil + sy, -pad + kx * dil + sx
            if mistake == 'dx_dil1' and ky == 0 and kx == 0:
                # the LAST tap of the dX conv (gather tap (KH - 1, KW - 1) = scatter tap (0, 0)) read at dilation 1:
                # iy = oy + [dil (K - 1) - pad] - (K - 1) instead of oy - pad
                oy_, ox_ = oy_ + (dil - 1) * (KH - 1), ox_ + (dil - 1) * (KW - 1)
            y0, y1 = max(0, -oy_), min(OH, Hs - oy_)
            x0, x1 = max(0, -ox_), min(OW, Ws - ox_)
            if y1 <= y0 or x1 <= x0:
                continue
            wt = w[:, wy, wx, :]
            c = (dz2 @ wt).view(B, OH, OW, Cin)
            a = (dz2.abs() @ wt.abs()).view(B, OH, OW, Cin)
            dx[:, y0 + oy_:y1 + oy_, x0 + ox_:x1 + ox_] += c[:, y0:y1, x0:x1]
            ab[:, y0 + oy_:y1 + oy_, x0 + ox_:x1 + ox_] += a[:, y0:y1, x0:x1]
    return dx, ab


def conv_backward_statement(x, w_eff, s, y, dy, relu, stride, pad, dil, mode, mistake=None):
    """x [B, H, W, Cin] (the Function's input), w_eff [Cout, KH, KW, Cin], s [Cout], y / dy [B, OH, OW, Cout]; mode 'bf16' / 'f16' /
    'f32' (None: no rounding anywhere, the f64 statement the CPU test holds against torch.autograd).
    -> dict(dz, dr, dx, dx_mag, dx_absxw, dx_K, dw, dw_mag, dw_absxw, dw_K, dt, ldp), f64; dw / dw_mag in parameter layout
    [Cout, Cin, KH, KW], dw_mag WITHOUT |s| (the bound multiplies it in); neither backward sum has a bias or residual term, so mag = absxw."""
    x, w, sd = R.values(x), R.values(w_eff, 'weight'), s.double()
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    assert (KH, KW) == (1, 1) or stride == 1
    xs = x[:, ::stride, ::stride, :]
    Hs, Ws = xs.shape[1], xs.shape[2]
    dz, dr = _dz(dy, y, relu, mode, mistake)
    OH, OW = dz.shape[1], dz.shape[2]
    assert (OH, OW) == out_hw(Hs, Ws, KH, 1, pad, dil)
    P = B * OH * OW
    step = kstep(mode)
    ldp = (P + step - 1) // step * step
    # ---- dX
    dxs, abs_ = _dx_scatter(dz, w, Hs, Ws, pad, dil, mistake)
    if stride > 1:
        dx, mag = (torch.zeros((B, H, W, Cin), dtype=torch.float64, device=x.device) for _ in range(2))
        mag[:, ::stride, ::stride] = abs_
        if mistake == 'stride_scatter_offset':                  # placed at (s oy + 1, s ox + 1), where that is inside the map
            sub = dx[:, 1::stride, 1::stride]
            sub.copy_(dxs[:, :sub.shape[1], :sub.shape[2]])
        else:
            dx[:, ::stride, ::stride] = dxs
    else:
        dx, mag = dxs, abs_
    # ---- dW
    cols, oh2, ow2 = R._patches(xs, KH, KW, 1, pad, dil, 'dil1' if mistake == 'wgrad_dil1' else None)    # [P, KH KW Cin]
    assert (oh2, ow2) == (OH, OW)
    dz2 = dz.reshape(P, Cout)
    rows = P
    if mistake == 'wgrad_last_slice_dropped':                   # the last K-step of 64 rows of P never enters the sum
        rows = (P - 1) // 64 * 64
    dwe = dz2[:rows].t() @ cols[:rows]
    dwa = dz2.abs().t() @ cols.abs()
    if mistake == 'pad_rows_live':
        # rows P .. ldp - 1 of BOTH operands hold 1.0 instead of zero (a finite value in one operand alone meets the other's zeros and
        # changes nothing; a non-finite one is what the GPU test's NaN-filled slabs are for)
        dwe = dwe + float(ldp - P)
    lay = lambda t: t.view(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    dw, dw_mag = lay(dwe), lay(dwa).contiguous()
    if mistake == 'wgrad_taps_swapped':
        dw = dw.transpose(2, 3)
    if mistake == 'wgrad_scale_by_cin':
        dw = dw * sd[torch.arange(Cin, device=sd.device) % Cout].view(1, Cin, 1, 1)
    elif mistake != 'wgrad_no_scale':
        dw = dw * sd.view(Cout, 1, 1, 1)
    return dict(dz=dz, dr=dr, dx=dx, dx_mag=mag, dx_absxw=mag, dx_K=KH * KW * Cout, dw=dw.contiguous(), dw_mag=dw_mag, dw_absxw=dw_mag, dw_K=P,
                dt=dz2.sum(0), ldp=ldp)


def linear_backward_statement(x, wc, y, dy, relu, mode, mistake=None):
    """x [M, K], wc [N, K] (the cast weight), y / dy [M, N] -> dict(dz, dr, dx, dx_mag, dx_K, dw, dw_mag, dw_K, db), f64."""
    x, w = R.values(x), R.values(wc, 'weight')
    M, Kd = x.shape
    N = w.shape[0]
    dz, dr = _dz(dy, y, relu, mode, mistake)
    dx, dx_mag = dz @ w, dz.abs() @ w.abs()
    if mistake == 'linear_dw_transposed':                       # x^T dz [K, N], its memory read as the parameter's [N, K]
        dw = (x.t() @ dz).contiguous().view(N, Kd)
    else:
        dw = dz.t() @ x
    db = dz.sum(0)
    if mistake == 'db_row_sums':                                # row sums laid into the [N] buffer (the first min(M, N) of them)
        rs = dz.sum(1)
        db = torch.zeros_like(db)
        db[:min(M, N)] = rs[:min(M, N)]
    dw_mag = dz.abs().t() @ x.abs()
    return dict(dz=dz, dr=dr, dx=dx, dx_mag=dx_mag, dx_absxw=dx_mag, dx_K=N, dw=dw, dw_mag=dw_mag, dw_absxw=dw_mag, dw_K=M, db=db)


# ------------------------------------------------------------------------------------------------ bounds
def _m(mode):
    return mode or 'f32'


def dx_bracket(st, mode):
    """[lo, hi] of the stored data gradient (one rounding of the f32 accumulator to the compute dtype)."""
    return R.stored_bracket(st['dx'], R.mfma_bound(st['dx_mag'], st['dx_absxw'], st['dx_K'], _m(mode)), _m(mode))


def dw_bound(st, mode, s=None, g0=None):
    """Bound on the f32 weight gradient (see the module docstring); s [Cout] for a conv; g0: the gradient it was added to."""
    b = R.mfma_bound(st['dw_mag'], st['dw_absxw'], st['dw_K'], _m(mode))
    if s is not None:
        b = b * s.double().abs().view(-1, *([1] * (b.dim() - 1)))
    if g0 is not None:
        b = b + SECOND * U * (g0.double().abs() + st['dw'].abs())
    return b


def colsum_bound(dz, g0=None):
    """(f64 column sums, bound) of the stored dz [.., N] as test_colsum_against_f64 holds hvr_colsum to; g0 as in dw_bound."""
    ref, b = K.colsum_bound(dz.reshape(-1, dz.shape[-1]))
    if g0 is not None:
        b = b + SECOND * U * (g0.double().abs() + ref.abs())
    return ref, b


def delivered(ref, g0, mistake=None):
    """What a gradient buffer that held g0 holds after the Function added `ref` into it ('accumulate_overwrites': wrote it)."""
    return ref if (g0 is None or mistake == 'accumulate_overwrites') else g0.double() + ref


def within(got, ref, bound):
    """-> (worst |got - ref| / bound, elements outside) for an f32 result."""
    r, bad, _ = R.compare(got, ref - bound, ref + bound, ref)
    return r, bad


# ------------------------------------------------------------------------------------------------ operand families
def conv_operands(name, mode, seed, exact=False):
    """CPU operands of CONV_CASES[name] as the Function takes them: x, resid, dy in the compute dtype (dy f32 when out_f32), the f32
    parameter w [Cout, Cin, k, k], scale s and shift t.  Real statistics: x after a ReLU, w ~ N(0, 1 / fan-in), s in [0.5, 1.5).
    exact: integers (|x|, |w| <= 15, |dy| <= 7) times q = 2^-4 (dy: times 1), s in {1/2, 1, 2}: every product of either backward sum is
    a multiple of q / 2 and the sums stay below 2^24 quanta (assert_exact_backward)."""
    (B, H, W, Cin, Cout, k, stride, pad, dil), relu, has_resid, out_f32 = CONV_CASES[name]
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = (H - 1) // stride + 1, (W - 1) // stride + 1
    OH, OW = out_hw(Hs, Ws, k, 1, pad, dil)
    dt = R.STORE[mode]
    if exact:
        q = 2.0 ** -4
        x = R._ints((B, H, W, Cin), -15, 15, g) * q
        w = R._ints((Cout, Cin, k, k), -15, 15, g) * q
        s = 2.0 ** R._ints((Cout,), -1, 1, g)
        t = R._ints((Cout,), -64, 64, g) * q
        resid = R._ints((B, OH, OW, Cout), -127, 127, g) * q
        dy = R._ints((B, OH, OW, Cout), -7, 7, g)
    else:
        x = torch.randn((B, H, W, Cin), generator=g).clamp(min=0.0)
        w = torch.randn((Cout, Cin, k, k), generator=g) / math.sqrt(Cin * k * k)
        s = torch.rand(Cout, generator=g) + 0.5
        t = torch.randn(Cout, generator=g) * 0.1
        resid = torch.randn((B, OH, OW, Cout), generator=g)
        dy = torch.randn((B, OH, OW, Cout), generator=g)
    return dict(x=x.to(dt), w=w.float(), s=s.float(), t=t.float(), resid=resid.to(dt) if has_resid else None,
                dy=dy.float() if out_f32 else dy.to(dt), relu=relu, out_f32=out_f32, stride=stride, pad=pad, dil=dil)


def linear_operands(name, mode, seed):
    M, Kd, N, relu, has_resid, has_bias, out_f32 = LINEAR_CASES[name]
    g = torch.Generator().manual_seed(seed)
    dt = R.STORE[mode]
    x = torch.randn((M, Kd), generator=g).clamp(min=0.0)
    w = torch.randn((N, Kd), generator=g) / math.sqrt(Kd)
    b = torch.randn(N, generator=g) * 0.1
    resid = torch.randn((M, N), generator=g)
    dy = torch.randn((M, N), generator=g)
    return dict(x=x.to(dt), w=w, b=b if has_bias else None, resid=resid.to(dt) if has_resid else None,
                dy=dy.float() if out_f32 else dy.to(dt), relu=relu, out_f32=out_f32)


def assert_exact_backward(st, s, mode):
    """The exact family's promise: both backward sums stay below 2^24 quanta (dX: multiples of q min(s) = 2^-5; dW: of q = 2^-4), so
    every partial sum in any order is an f32 number; s is a power of two; dX stays inside the 16-bit format's range."""
    assert bool((torch.log2(s.double()) == torch.log2(s.double()).round()).all())
    assert float(st['dx_mag'].max()) <= 2.0 ** 24 * 2.0 ** -5 and float(st['dw_mag'].max()) <= 2.0 ** 24 * 2.0 ** -4
    assert bool((st['dx'] * 32 == (st['dx'] * 32).round()).all()) and bool((st['dw'].float().double() == st['dw']).all())
    if mode == 'f16':
        assert float(st['dx'].abs().max()) < 65504.0


def stored_y(o, w_eff, mode):
    """The stored forward output of a conv case on the host (what the GPU test reads off the Function): RN of the f64 forward
    statement -- for the CPU tests, which need a gate."""
    r = None if o['resid'] is None else o['resid'].double()
    y = R.conv_statement(o['x'].double(), w_eff.double(), o['t'].double(), r, o['relu'], o['stride'], o['pad'], o['dil'])[0]
    return y.float().double() if (o['out_f32'] or mode == 'f32') else R.round_stored(y, mode)


def conv_statement_of(o, w_eff, y, mode, mistake=None):
    return conv_backward_statement(o['x'], w_eff, o['s'], y, o['dy'], o['relu'], o['stride'], o['pad'], o['dil'], mode, mistake)
