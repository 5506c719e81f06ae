"""Plain float64 statement of the deformable-conv sampler (hvr_deform_im2col, DCN v1 / v2), written from the rule the C ABI states
(include/hvr_hip.h) independently of the HIP code, with the error bound that tests/test_dcn_refs.py (CPU) and tests/test_dcn_gpu.py
(GPU) hold the kernel to.  Style and constants of tests/forward_kernel_refs.py / tests/train_loss_refs.py.

The rule.  x [B, H, W, Cin] (stored values), om [B, OH, OW, ldo] f32 (offsets, then mask logits when modulated).  For output pixel
(b, oy, ox), tap k = kh KW + kw and channel c of deformable group g = c // (Cin / dg):
    off_h = om[g 2 KH KW + 2 k],  off_w = om[g 2 KH KW + 2 k + 1],  logit = om[2 dg KH KW + g KH KW + k]
    h = fl32(float(oy stride - pad + kh dil) + off_h),  w alike          <- the ONLY f32 step of the statement (torch f32, CPU)
    sample = 0 unless h > -1, w > -1, h < H, w < W
    else     sum over the corners (floor h | floor h + 1) x (floor w | floor w + 1) of weight . value, a corner outside
             [0, H - 1] x [0, W - 1] contributing 0 (no edge clamp)
    col[(b, oy, ox), k Cin + c] = sample (. sigmoid(logit) when modulated)
Everything after the position add is float64.

Bound on the f32 value the kernel holds before its store, per element: (c u + S u [modulated]) sum_k |w_k| |v_k| (. mask), first
order, times SECOND.  c counts the f32 roundings behind one term of the sum when no operation is fused (the file is built with
-ffp-contract=off):
    C_AXIS_H = 1   hh = 1 - lh            (lh = h - floor(h) is exact: both are f32 numbers of one binade or h's is coarser)
    C_AXIS_W = 1   hw = 1 - lw
    C_WEIGHT = 1   the weight product hh hw (or hh lw, lh hw, lh lw)
    C_PRODUCT = 1  weight . value
    C_ADDS = 3     three additions join four products; in ANY association a term passes through at most three of them
    C_SLACK = 1    one unit in hand for lh itself, should an implementation form it from a rounded intermediate
  c = 8, and C_MASK = 1 more for the product with the mask when modulated.
The mask 1 / (1 + expf(-logit)): expf's relative error EXPF_ULP ulp = 2 EXPF_ULP u (train_loss_refs.py: no accuracy table of the
device math library ships with the ROCm documentation installed next to the compiler, so the OpenCL full-profile limit of the
same built-in, 3 ulp, is used, as for every other device exponential of this suite) reaches the quotient damped by
e / (1 + e) <= 1; the addition and the division are correctly rounded (`hipcc --help`: -fhip-fp32-correctly-rounded-divide-sqrt,
"Specify that single precision floating-point divide and sqrt used in the program source are correctly rounded (HIP device
compilation only)", on by default): u each.  S = 2 EXPF_ULP + 2 = 8.  A fast intrinsic (__expf) has no documented accuracy and is
not covered.  No bound contains a value measured on the device.

Stored output: bf16 / half: ONE rounding of the f32 value (train_loss_refs.bracket); split half: the SPLIT_REL / SPLIT_ABS rule of
forward_kernel_refs.stored_bracket; f32: the bound itself.

`mistake=`: plausible kernel mistakes stated exactly (MISTAKES); tests/test_dcn_refs.py shows each outside the bound on
real-statistics inputs or unequal on the exact families.
"""
import torch

from tests import forward_kernel_refs as F
from tests import train_loss_refs as L

U = L.U
SECOND = L.SECOND
C_AXIS_H, C_AXIS_W, C_WEIGHT, C_PRODUCT, C_ADDS, C_SLACK, C_MASK = 1, 1, 1, 1, 3, 1, 1
C_ROUNDINGS = C_AXIS_H + C_AXIS_W + C_WEIGHT + C_PRODUCT + C_ADDS + C_SLACK          # 8
S_SIGMOID = 2 * L.EXPF_ULP + 2                                                       # expf, then a correctly rounded add and divide
SENTINEL = F.SENTINEL

MISTAKES = ('hw_swapped', 'border_closed', 'corner_clamped', 'group_ignored', 'mask_first_channels', 'tap_transposed', 'dil1',
            'stride1', 'rows_past_M', 'mask_unapplied')


def out_hw(H, W, KH, KW, stride, pad, dil):
    return (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1


def sampler_statement(x, om, KH, KW, stride, pad, dil, dg, modulated, mistake=None):
    """x [B, H, W, Cin] true stored values (any float dtype), om [B, OH, OW, ldo] f32 -> (ref, bound) f64 [B OH OW, KH KW Cin], the
    bound on the f32 value before the store.  Runs on the CPU.  Mistakes:
      hw_swapped           the two offset channels of a tap read in the other order
      border_closed        the sample dropped unless h >= 0 and w >= 0 (the reference's commented-out test)
      corner_clamped       a corner outside the map read from the clamped (edge) pixel, as RoIAlign does
      group_ignored        every channel uses group 0's offsets and mask
      mask_first_channels  the mask logit read at g KH KW + k (the first channels) instead of behind the 2 dg KH KW offsets
      tap_transposed       tap (kh, kw) reads the offsets and mask of tap (kw, kh)
      dil1                 the last tap placed at dilation 1
      stride1              the pixel grid placed at stride 1
      mask_unapplied       the mask never multiplied in
    ('rows_past_M' is a store mistake: forward_kernel_refs.emulate_store)"""
    x = x.detach().cpu().double()
    om = om.detach().cpu().float()
    B, H, W, C = x.shape
    OH, OW = out_hw(H, W, KH, KW, stride, pad, dil)
    assert tuple(om.shape[:3]) == (B, OH, OW) and C % dg == 0
    KK = KH * KW
    cpg = C // dg
    assert om.shape[3] >= (3 if modulated else 2) * dg * KK
    oy = torch.arange(OH)[None, :, None].expand(B, OH, OW)
    ox = torch.arange(OW)[None, None, :].expand(B, OH, OW)
    bi = torch.arange(B)[:, None, None].expand(B, OH, OW)
    ref = torch.zeros((B, OH, OW, KK, C), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    st = 1 if mistake == 'stride1' else stride
    for kh in range(KH):
        for kw in range(KW):
            k = kh * KW + kw
            ko = (kw * KH + kh) if (mistake == 'tap_transposed' and KH == KW) else k
            d = 1 if (mistake == 'dil1' and k == KK - 1) else dil
            base_h = (oy * st - pad + kh * d).float()                  # integer arithmetic, then the conversion (exact)
            base_w = (ox * st - pad + kw * d).float()
            for g in range(dg):
                go = 0 if mistake == 'group_ignored' else g
                ch, cw = go * 2 * KK + 2 * ko, go * 2 * KK + 2 * ko + 1
                if mistake == 'hw_swapped':
                    ch, cw = cw, ch
                h = (base_h + om[..., ch]).double()                    # ONE f32 add each
                w = (base_w + om[..., cw]).double()
                if mistake == 'border_closed':
                    inside = (h >= 0) & (w >= 0) & (h < H) & (w < W)
                else:
                    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
                hl, wl = torch.floor(h), torch.floor(w)
                lh, lw = h - hl, w - wl
                val = torch.zeros((B, OH, OW, cpg), dtype=torch.float64)
                m = torch.zeros_like(val)
                for dy, wy in ((0, 1 - lh), (1, lh)):
                    for dx, wx in ((0, 1 - lw), (1, lw)):
                        yi, xi = hl + dy, wl + dx
                        ok = (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)
                        if mistake == 'corner_clamped':
                            ok = torch.ones_like(ok)
                        v = x[bi, yi.clamp(0, H - 1).long(), xi.clamp(0, W - 1).long(), g * cpg:(g + 1) * cpg]
                        v = v * (ok & inside)[..., None]
                        wgt = (wy * wx)[..., None]
                        val = val + wgt * v
                        m = m + wgt.abs() * v.abs()
                if modulated and mistake != 'mask_unapplied':
                    cm = (go * KK + ko) if mistake == 'mask_first_channels' else (2 * dg * KK + go * KK + ko)
                    mask = torch.sigmoid(om[..., cm].double())[..., None]
                    val, m = val * mask, m * mask
                ref[:, :, :, k, g * cpg:(g + 1) * cpg] = val
                mag[:, :, :, k, g * cpg:(g + 1) * cpg] = m
    coef = C_ROUNDINGS + ((C_MASK + S_SIGMOID) if modulated else 0)
    bound = SECOND * coef * U * mag
    return ref.view(B * OH * OW, KK * C), bound.view(B * OH * OW, KK * C)


def stored_bracket(ref, bound, mode):
    return F.stored_bracket(ref, bound, mode)


def real_inputs(B, H, W, C, KH, KW, stride, pad, dil, dg, modulated, mode, seed, ldo=None, spread=1.5):
    """Real-statistics inputs: x after a ReLU (half zeros, |N(0, 1)|) rounded to what `mode` stores (f64 true values); offsets
    N(0, spread) pixels (so the map's border is crossed in both directions), mask logits N(0, 2); om [B, OH, OW, ldo] f32 with
    NaN-free filler in the unused columns (a kernel that reads them lands far outside the bound)."""
    g = torch.Generator().manual_seed(seed)
    x = F.store_true(torch.randn((B, H, W, C), generator=g).clamp(min=0.0), mode, 'act')
    OH, OW = out_hw(H, W, KH, KW, stride, pad, dil)
    n = (3 if modulated else 2) * dg * KH * KW
    ldo = n if ldo is None else ldo
    om = torch.full((B, OH, OW, ldo), 1000.0)
    om[..., :2 * dg * KH * KW] = torch.randn((B, OH, OW, 2 * dg * KH * KW), generator=g) * spread
    if modulated:
        om[..., 2 * dg * KH * KW:n] = torch.randn((B, OH, OW, dg * KH * KW), generator=g) * 2.0
    return x, om


def exact_inputs(B, H, W, C, KH, KW, stride, pad, dil, dg, modulated, mode, seed, family, ldo=None):
    """Inputs on which every f32 operation of a correct kernel is exact, so the stored result must EQUAL round-to-nearest of the
    statement.  Values are integers of <= 5 bits x 2^-4 (lo_act, split half: up to 13-bit integers, a non-zero lo half); weights
    from offsets that are multiples of 1/8 are multiples of 1/64, products and their sums stay below 2^24 quanta.  family:
      'zero'      zero offsets: col is the index-arithmetic im2col
      'integer'   integer offsets in [-H - 2, H + 2] (reaching outside the map on every side)
      'eighths'   offsets that are multiples of 1/8 in [-3, 3]
      'border'    positions exactly -1, in (-1, 0), exactly H - 1 (W - 1), in (H - 1, H), and exactly H (W), by cycling per pixel
      'lo_act'    'eighths' on wide split-half values (the lo plane must be read and written)
    modulated: logits cycle through {0, +32, -128}: masks exactly 0.5, 1 and 0 under any correct f32 sigmoid."""
    g = torch.Generator().manual_seed(seed)
    q = 2.0 ** -4
    top = (2 ** 13 - 1) if family == 'lo_act' else 31
    x = torch.randint(-top, top + 1, (B, H, W, C), generator=g).double() * q
    assert bool((F.store_true(x.float(), mode, 'act') == x).all())
    OH, OW = out_hw(H, W, KH, KW, stride, pad, dil)
    KK = KH * KW
    n = (3 if modulated else 2) * dg * KK
    ldo = n if ldo is None else ldo
    om = torch.full((B, OH, OW, ldo), 1000.0)
    shp = (B, OH, OW, 2 * dg * KK)
    if family == 'zero':
        off = torch.zeros(shp)
    elif family == 'integer':
        off = torch.randint(-max(H, W) - 2, max(H, W) + 3, shp, generator=g).float()
    elif family in ('eighths', 'lo_act'):
        off = torch.randint(-24, 25, shp, generator=g).float() / 8.0
    else:
        assert family == 'border'
        off = torch.zeros(shp)
        oy = torch.arange(OH)[None, :, None].expand(B, OH, OW)
        ox = torch.arange(OW)[None, None, :].expand(B, OH, OW)
        for gk in range(dg * KK):
            k = gk % KK
            kh, kw = k // KW, k % KW
            by = (oy * stride - pad + kh * dil).float()
            bx = (ox * stride - pad + kw * dil).float()
            sel = (oy * OW + ox + gk) % 10
            ty = torch.tensor([-1.0, -0.375, H - 1.0, H - 0.625, float(H), 1.25, 0.0, 2.5, -1.0, H - 0.125])[sel]
            tx = torch.tensor([0.5, 1.0, 0.0, 2.25, 1.0, -1.0, -0.625, W - 1.0, W - 0.375, float(W)])[sel]
            off[..., 2 * gk] = ty - by
            off[..., 2 * gk + 1] = tx - bx
    om[..., :2 * dg * KK] = off
    if modulated:
        idx = torch.randint(0, 3, (B, OH, OW, dg * KK), generator=g)
        om[..., 2 * dg * KK:n] = torch.tensor([0.0, 32.0, -128.0])[idx]
    return x, om


def to_device_operand(x, mode, device):
    """True f64 values -> the tensor a kernel of `mode` reads (split half: the x 16 container)."""
    from hvrnet_amd import native
    xf = x.float().to(device)
    if mode == 'f16x2':
        return native.cast(xf, native.SPLIT)
    return xf.to(F.STORE[mode]).contiguous()
