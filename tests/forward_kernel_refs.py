"""Plain float64 statements of the FORWARD kernels -- convs (hvr_conv2d_nhwc, all routes), products (hvr_gemm), the fused
Bottleneck tails (hvr_bottleneck_tail / _tail_next), the stem (hvr_stem_fused, hvr_im2col_stem, hvr_maxpool3x3s2_nhwc) and the
relation core (hvr_relation_fwd / _grouped) -- written independently of the HIP code and of torch's conv dispatch, with the error
bounds that tests/test_forward_kernel_refs.py (CPU) and tests/test_forward_kernels_gpu.py (GPU) hold the kernels to.

Operands enter as STORED values (`values`): bf16 / half / f32 tensors as they are, split-half containers (native.SPLIT) through
native.cast(., float32) with the x 16 activation / x 64 weight scales of native.py removed.  A statement is the exact function of
those values, in float64; every function works on the CPU and on the device, and the callers feed one frame (or one row chunk) at
a time, so the f64 patch matrix of layer 1 at 60 frames never exists whole.

Error model (as tests/train_loss_refs.py): u = U = 2^-24.  `mag` = sum|x||w| + |bias| + |resid| per output element.
  f32 MFMA        (K + e) u mag: cdna_hip_programming.md documents v_mfma_f32_*_f32 as a k-ordered f32 fma chain, one rounding per
                  product; a sum of K terms in ANY order (K slices, split-K partials, wave partials included) whose longest chain
                  is c has error <= c u sum|term|, and c <= K; e = E_EPI counts the epilogue's f32 operations (alpha, + bias,
                  + residual).
  bf16 / half     (K + e) 2u mag: the products are exact in f32; the guides do not document how the matrix core rounds its
                  internal multi-term sum, so every added term is allowed 2u instead of u.  This allowance covers an MFMA that
                  TRUNCATES its internal sums (truncation = at most one ulp = 2u per addition).
  split half      three half MFMAs per product (hi hi + hi lo + lo hi): 3K added terms at 2u each, plus 2^-22 sum|x||w| for the
                  dropped lo lo products (|lo| <= 2^-11 |x|), plus, on store, the absolute allowance of a lo half in half's subnormal
                  range that the comment of hvr_gemm_desc.alpha describes (SPLIT_ABS, below).
  tile hint 18    (include/hvr_hip.h "tile_hint 18 ... TWO-LEVEL accumulation"): blocks of kTwoLevelSteps = 8 K-steps of 32 elements
                  sum on their own and are then added to the running total: the chain is 256 + K / 256 instead of K.
  stored output   a 16-bit result is ONE rounding of the f32 value: it must lie in the bracket [RN(ref - bound), RN(ref + bound)]
                  (train_loss_refs.bracket); a split-half result is rounded to hi + lo: 2^-22 relative + SPLIT_ABS.
All bounds are first order, multiplied by SECOND = 1 + 2^-10.  No bound contains a value measured on the device.

Each statement takes `mistake=`: a plausible kernel mistake stated exactly (MISTAKES); the CPU tests show every one of them
outside the bound / bracket on real-statistics operands or unequal on the exact-sum operands (`exact_*` builders: every value a
multiple of a quantum q, mag <= 2^24 q^2, so every partial sum is exact in f32 in any order and the kernel must return
round-to-nearest-even of the statement).
"""
import math

import torch

from tests import train_loss_refs as L

U = L.U
SECOND = L.SECOND
E_EPI = 3                      # alpha * acc, + beta * bias, + residual: at most three f32 operations behind the accumulator
ACT_SCALE, WEIGHT_SCALE = 16.0, 64.0     # native.SPLIT_ACT_SCALE / SPLIT_WEIGHT_SCALE (asserted equal by the GPU test)
SPLIT_REL = 2.0 ** -22         # hi + lo keeps 22 significant bits (include/hvr_hip.h, HVR_F16S)
SPLIT_ABS = 2.0 ** -24 / ACT_SCALE   # "absolute error < 2^-24 below [2^-3]" (HVR_F16S; hvr_gemm_desc.alpha), in true units of a x 16 activation
TWO_LEVEL_BLOCK = 256          # kTwoLevelSteps (8) K-steps of 32 elements (gemm.hip two_level_supported: (K / 32) % 8 == 0)
SENTINEL = 7777.0              # what output buffers hold before a call (exact in every format; no statement produces it)
MODES = ('bf16', 'f16', 'f16x2', 'f32')
STORE = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}

MISTAKES = ('k_drop', 'k_twice', 'tap_border', 'dil1', 'rows_past_M', 'skip_last_tile', 'bias_last_chunk', 'resid_after_relu',
            'shortcut_odd', 'hn_unrounded', 'trunc_store', 'no_hi_lo', 'no_lo_hi', 'alpha_on_bias', 'block_weight_skipped',
            'group_offset')


def mode_of(dtype):
    return {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32', torch.int32: 'f16x2'}[dtype]


def values(t, role='act'):
    """The stored values of an operand as f64.  role: 'act' (split half: x 16 removed) or 'weight' (x 64 removed)."""
    if t is None:
        return None
    if t.dtype == torch.int32:                                   # the split-half container
        from hvrnet_amd import native
        return native.cast(t, torch.float32, scale=1.0 / (ACT_SCALE if role == 'act' else WEIGHT_SCALE)).double()
    return t.double()


def split_parts(v, scale):
    """(hi, lo) of the split-half storage of the true values v (f64) kept x scale: hi = half(s v), lo = half(s v - hi), in units of v."""
    s = v * scale
    hi = s.to(torch.float16).double()
    lo = (s - hi).to(torch.float16).double()
    return hi / scale, lo / scale


def split_round(v, scale=ACT_SCALE):
    hi, lo = split_parts(v, scale)
    return hi + lo


def round_stored(v, mode):
    """RN of f64 values to the stored format of `mode` (f64 -> f32 -> 16 bits rounds twice: the callers use it on values that are
    f32 numbers already, or compare through brackets)."""
    if mode == 'f16x2':
        return split_round(v)
    return v.float().to(STORE[mode]).double()


def truncate_stored(v, mode):
    """Truncation (round toward zero) of f32-exact values to bf16 / half (normal range): the 'trunc_store' mistake, by clearing the
    f32 mantissa bits the format does not keep."""
    drop = {'bf16': 16, 'f16': 13}[mode]
    bits = v.float().contiguous().view(torch.int32)
    return ((bits >> drop) << drop).view(torch.float32).double()


# ------------------------------------------------------------------------------------------------ bounds
def chain(K, mode, two_level=False):
    """Longest chain of additions behind one accumulator."""
    per = 3 if mode == 'f16x2' else 1
    if two_level:
        assert K % TWO_LEVEL_BLOCK == 0 and mode in ('f32', 'f16x2')
        return per * TWO_LEVEL_BLOCK + K // TWO_LEVEL_BLOCK
    return per * K


def mfma_bound(mag, absxw, K, mode, two_level=False):
    """Bound on the f32 value a kernel holds before its store (see the module docstring)."""
    c = chain(K, mode, two_level) + E_EPI
    b = c * (U if mode == 'f32' else 2 * U) * mag
    if mode == 'f16x2':
        b = b + SPLIT_REL * absxw
    return SECOND * b


def stored_bracket(ref, bound, mode, out_f32=False):
    """[lo, hi] the stored result must lie in."""
    if out_f32 or mode == 'f32':
        return ref - bound, ref + bound
    if mode == 'f16x2':
        b = bound + SECOND * SPLIT_REL * (ref.abs() + bound) + SPLIT_ABS
        return ref - b, ref + b
    return L.bracket(ref, bound, STORE[mode])


# ------------------------------------------------------------------------------------------------ conv / gemm statements
def _patches(x, KH, KW, stride, pad, dil, mistake=None):
    """x [B, H, W, C] f64 -> patch matrix [B * OH * OW, KH * KW * C] by plain index arithmetic (zero outside the map), OH, OW."""
    B, H, W, C = x.shape
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    oy = torch.arange(OH, device=x.device)[:, None]
    ox = torch.arange(OW, device=x.device)[None, :]
    cols = torch.zeros((B, OH, OW, KH * KW, C), dtype=torch.float64, device=x.device)
    for ky in range(KH):
        for kx in range(KW):
            d = 1 if (mistake == 'dil1' and ky == KH - 1 and kx == KW - 1) else dil   # 'dil1': the last tap read at dilation 1
            iy = oy * stride - pad + ky * d + 0 * ox
            ix = ox * stride - pad + kx * d + 0 * oy
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            if mistake == 'tap_border' and ky == KH // 2 and kx == KW // 2:      # the centre tap masked at the right / bottom border only
                ok = ok & (ox < OW - 1) & (oy < OH - 1)
            v = x[:, iy.clamp(0, H - 1), ix.clamp(0, W - 1), :]
            cols[:, :, :, ky * KW + kx, :] = v * ok[None, :, :, None]
    return cols.view(B * OH * OW, KH * KW * C), OH, OW


def _product(a, w, mistake, mode):
    """a [M, K] . w [N, K]^T in f64 with the K-loop mistakes, and sum|a||w|."""
    K = a.shape[1]
    absxw = a.abs() @ w.abs().t()
    if mistake == 'k_drop':                                       # last K-step of 32 dropped
        acc = a[:, :K - 32] @ w[:, :K - 32].t()
    elif mistake == 'k_twice':                                    # ... applied twice
        acc = a @ w.t() + a[:, K - 32:] @ w[:, K - 32:].t()
    elif mistake in ('no_hi_lo', 'no_lo_hi'):
        ah, al = split_parts(a, ACT_SCALE)
        wh, wl = split_parts(w, WEIGHT_SCALE)
        acc = ah @ wh.t() + (al @ wh.t() if mistake == 'no_hi_lo' else ah @ wl.t())
    else:
        acc = a @ w.t()
    return acc, absxw


def _epilogue(acc, absxw, bias, resid, relu, mistake):
    """act(acc + bias + resid) and mag, with the epilogue mistakes.  acc / absxw [M, N], bias [N], resid [M, N] (f64 or None)."""
    M, N = acc.shape
    mag = absxw.clone()
    y = acc
    if mistake == 'alpha_on_bias' and bias is not None:           # split half: alpha (1 / 64 on a scaled output) applied to the bias as well
        bias = bias / WEIGHT_SCALE
    if bias is not None:
        b = bias.double().clone()
        if mistake == 'bias_last_chunk':
            b[max(0, N - 64):] = 0.0
        y = y + b[None, :]
        mag = mag + bias.double().abs()[None, :]
    if resid is not None:
        mag = mag + resid.abs()
        if mistake != 'resid_after_relu':
            y = y + resid
    if relu:
        y = y.clamp(min=0.0)
    if resid is not None and mistake == 'resid_after_relu':
        y = y + resid
    if mistake == 'skip_last_tile':                               # the last (persistent) tile of 128 rows never written
        y = y.clone()
        y[(M - 1) // 128 * 128:] = SENTINEL
    return y, mag


def gemm_statement(a, w, bias=None, resid=None, relu=False, mistake=None, mode=None):
    """act(a [M, K] . w [N, K]^T + bias + resid) -> (ref, mag, sum|a||w|), all f64 [M, N]."""
    acc, absxw = _product(a.double(), w.double(), mistake, mode)
    ref, mag = _epilogue(acc, absxw, bias, None if resid is None else resid.double(), relu, mistake)
    return ref, mag, absxw


def conv_statement(x, w, bias=None, resid=None, relu=False, stride=1, pad=0, dil=1, mistake=None, mode=None):
    """x [B, H, W, Cin], w [Cout, KH, KW, Cin], bias [Cout], resid [B, OH, OW, Cout] -> (ref, mag, sum|x||w|) f64 [B, OH, OW, Cout]:
    im2col by index arithmetic, then one f64 product."""
    Cout, KH, KW, Cin = w.shape
    cols, OH, OW = _patches(x.double(), KH, KW, stride, pad, dil, mistake)
    B = x.shape[0]
    r = None if resid is None else resid.double().reshape(B * OH * OW, Cout)
    ref, mag, absxw = gemm_statement(cols, w.double().reshape(Cout, KH * KW * Cin), bias, r, relu, mistake, mode)
    shp = (B, OH, OW, Cout)
    return ref.view(shp), mag.view(shp), absxw.view(shp)


def tail_statement(h, x, w, bias, stride2=1, relu=True, mistake=None, mode=None):
    """relu(h W3^T + x_s Wd^T + b): h [B, OH, OW, C1], x [B, H2, W2, C2] sampled every stride2-th pixel, w [Cout, C1 + C2] = [W3 | Wd]."""
    B, OH, OW, C1 = h.shape
    off = 1 if (mistake == 'shortcut_odd' and stride2 == 2) else 0     # the stride-2 shortcut sampled at odd pixels
    xs = x.double()[:, off::stride2, off::stride2, :][:, :OH, :OW, :]
    if xs.shape[1] < OH or xs.shape[2] < OW:                            # (odd sampling runs off an odd-sized map: clamp)
        xs = torch.nn.functional.pad(xs, (0, 0, 0, OW - xs.shape[2], 0, OH - xs.shape[1]))
    a = torch.cat([h.double(), xs], 3).reshape(B * OH * OW, C1 + x.shape[3])
    ref, mag, absxw = gemm_statement(a, w.double(), bias, None, relu, mistake, mode)
    shp = (B, OH, OW, w.shape[0])
    return ref.view(shp), mag.view(shp), absxw.view(shp)


def tail_next_statement(h, x, resid, w, bias, wn, bias_n, stride2=1, mode='bf16', mistake=None):
    """y = relu(h W3^T [+ x_s Wd^T] + b [+ resid]) and hn = relu(RN(y) wn^T + bn).  RN is the rounding to the STORED format of y
    (bf16 / half: round to nearest even; split half: hi + lo), because the kernel feeds the stored y to the next conv1 -- the
    tile it keeps for that product is the tile it writes.  -> dict(y=(ref, mag, absxw), y_stored, hn=(ref, mag, absxw)); the
    caller adds |y_got - RN(y_ref)| . |wn| to hn's bound (hn_extra)."""
    if x is not None:
        y = tail_statement(h, x, w, bias, stride2, True, mistake, mode)
    else:
        B, OH, OW, C1 = h.shape
        r = gemm_statement(h.double().reshape(-1, C1), w.double(), bias, resid.double().reshape(B * OH * OW, -1), True, mistake, mode)
        y = tuple(t.view(B, OH, OW, -1) for t in r)
    ys = y[0] if mistake == 'hn_unrounded' else round_stored(y[0], mode)
    Cout = w.shape[0]
    hn = gemm_statement(ys.reshape(-1, Cout), wn.double(), bias_n, None, True, None, mode)
    shp = ys.shape[:3] + (wn.shape[0],)
    return dict(y=y, y_stored=ys, hn=tuple(t.view(shp) for t in hn))


def hn_extra(y_lo, y_hi, y_stored, wn):
    """The allowance of hn for a stored y that differs from RN(y_ref) inside its bracket: max|y - RN(y_ref)| . |wn|^T."""
    dy = torch.maximum(y_hi - y_stored, y_stored - y_lo).clamp(min=0.0)
    return (dy.reshape(-1, dy.shape[-1]) @ wn.double().abs().t()).view(dy.shape[:3] + (wn.shape[0],))


def maxpool_statement(x):
    """nn.MaxPool2d(3, 2, 1) on [B, H, W, C] f64 (taps outside the map are skipped)."""
    B, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    p = torch.full((B, H + 2, W + 2, C), -float('inf'), dtype=x.dtype, device=x.device)
    p[:, 1:H + 1, 1:W + 1] = x
    out = torch.full((B, OH, OW, C), -float('inf'), dtype=x.dtype, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, p[:, dy:dy + 2 * OH - 1:2, dx:dx + 2 * OW - 1:2])
    return out


def im2col_stem_statement(img, kp):
    """hvr_im2col_stem: img [B, 3, H, W] -> [B * OH * OW, kp], column (ky * 7 + kx) * 3 + c, zero from 147 on."""
    cols, OH, OW = _patches(img.double().permute(0, 2, 3, 1), 7, 7, 2, 3, 1)
    out = torch.zeros((cols.shape[0], kp), dtype=torch.float64, device=img.device)
    out[:, :147] = cols
    return out, OH, OW


def stem_statement(img, w, bias, mode, mistake=None):
    """hvr_stem_fused: conv 7x7/2 (pad 3) + bias + ReLU + maxpool 3x3/2 (pad 1).  img [B, 3, H, W] f32; w [64, 7, 7, 3], bias [64] true
    values.  Roundings the kernel applies, stated: (1) the image is rounded to the operand format when it is laid out in the LDS
    (stem.hip: "rounded to bf16"; split half: to hi + lo, 22 bits -- carried in the bound as SPLIT_REL sum|x||w| + 2^-25 sum|w| for a
    lo half in half's subnormal range, the images being unscaled); (2) bf16 / half: every conv pixel is rounded to the format
    BEFORE the pool (stem.hip: "written (bias, ReLU, bf16) to LDS and max-pooled from there").  Rounding is monotone, so it commutes
    with the maximum and the pooled value is the one rounding of max(conv): |max a - max b| <= max|a - b| carries the conv bound through
    the pool.  -> (ref, bound) of the pooled f32 value before its store, [B, PH, PW, 64]."""
    x = img.double().permute(0, 2, 3, 1)
    if mode in ('bf16', 'f16'):
        x = round_stored(x, mode)
    ref, mag, absxw = conv_statement(x, w, bias, None, True, 2, 3, 1, mistake, mode)
    bound = mfma_bound(mag, absxw, 7 * 32, mode)                  # the kernel's K: 7 rows of 8 taps x 4 channels, zero padded
    if mode == 'f16x2':
        bound = bound + SECOND * (SPLIT_REL * absxw + 2.0 ** -25 * w.double().abs().sum((1, 2, 3))[None, None, None, :])
    return maxpool_statement(ref), maxpool_statement(bound)


# ------------------------------------------------------------------------------------------------ relation core
INTEGER_MAXIMA_TERMS = 2       # the numerator's exponent and the denominator's: each carries the < 1 (log2) larger gap of an integer block maximum


def relation_statement(q, k, v, scale, mode, grouped_apply=False, mistake=None):
    """softmax(scale q k^T) v in f64 -> (ref, bound) on the f32 value before the store, [Mq, D].  Built on
    train_loss_refs.relation_probs_statement (P and its bound for f32 dot products); added terms, each named after its source:
      dot_allowance   bf16 / half products: 2u per added term (module docstring), split half 3 D terms + SPLIT_REL: E_s grows by
                      (c - 1) E_s, entering as P (1 - P) (expm1(2 c E_s) - expm1(2 E_s));
      ptilde_format   DESIGN.md "Relation workspace ... P~ [Mq][ldp] (operand dtype)" / "whose intermediate is the bf16 probability
                      matrix P~": P~ is rounded to the operand format between the two passes: u_T (P + bound), + 2^-25 per key for half's
                      subnormal range (train_loss_refs.SUBNORMAL_HALF_STEP);
      integer_maxima  DESIGN.md "the scores pass rounds its block maxima up to integers so the block weights are exact powers of two,
                      applied on the exponent fields of the P~ fragments" (grouped apply pass): every exponent gap grows by < 1 (log2
                      units) -> 4 u ln2 more on P's own exponent error AND 4 u ln2 more on the denominator's (the `4 u gap` and
                      `4 u G` terms of relation_probs_statement, one each: INTEGER_MAXIMA_TERMS = 2); bf16 fragments whose weighted exponent leaves the format are clamped
                      below 2^-126 (TINY per key); split half (include/hvr_hip.h, hvr_relation_fwd_grouped: "up to the half rounding of
                      block-weighted probabilities below 2^-26 of a row's largest"): 2^-26 max_j P per key;
      apply_sum       O = sum_j P_j v_j on the matrix cores: (ldp + 2 nt + E_EPI) added terms (keys, block joins, block factors) at u
                      (f32) / 2u (bf16, half) / 3 x 2u + SPLIT_REL (split half) of sum_j P_j |v_j|.
    mistake 'block_weight_skipped': the second 128-key block (the last when there is one) enters without its weight 2^(m_t - m*)."""
    Mq, D = q.shape
    Mk = k.shape[0]
    qd, kd, vd = q.double(), k.double(), v.double()
    P, bP, nt = L.relation_probs_statement(qd, kd, scale)
    P, bP = P[:, :Mk], bP[:, :Mk]
    sc = L.f32v(scale)
    absdot = qd.abs() @ kd.abs().t()
    gD = D * U / (1 - D * U)
    Es = (sc * gD * absdot).max(1).values[:, None]
    c = {'f32': 1.0, 'bf16': 2.0, 'f16': 2.0, 'f16x2': 6.0}[mode]
    Es2 = c * Es + (sc * SPLIT_REL * absdot.max(1).values[:, None] if mode == 'f16x2' else 0.0)
    top = P.argmax(1, keepdim=True)
    om = (1 - P).scatter(1, top, P.scatter(1, top, 0.0).sum(1, keepdim=True))
    dP = bP + SECOND * P * om * (torch.expm1(2 * Es2) - torch.expm1(2 * Es))                       # dot_allowance
    uT = {'f32': U, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11, 'f16x2': SPLIT_REL}[mode]
    dP = dP + uT * (P + dP) + (2.0 ** -25 if mode in ('f16', 'f16x2') else 0.0)                   # ptilde_format
    if grouped_apply:                                                                              # integer_maxima
        assert mode in ('bf16', 'f16x2'), 'the grouped apply pass is stated for the modes the census runs it in'
        dP = dP + SECOND * P * INTEGER_MAXIMA_TERMS * 4 * U * math.log(2.0) + L.TINY
        if mode == 'f16x2':
            dP = dP + 2.0 ** -26 * P.max(1, keepdim=True).values
    if mistake == 'block_weight_skipped':
        t = 1 if nt > 1 else 0
        S = sc * (qd @ kd.t())
        mstar = S.max(1, keepdim=True).values
        blk = S[:, 128 * t:128 * (t + 1)]
        e = torch.exp(S - mstar)
        Lsum = e.sum(1, keepdim=True)
        e[:, 128 * t:128 * (t + 1)] = torch.exp(blk - blk.max(1, keepdim=True).values)
        P = e / Lsum
    absv = vd.abs()
    ref = P @ vd
    terms = (nt * 128 + 2 * nt + E_EPI) * (3 if mode == 'f16x2' else 1)
    PV = P @ absv
    bound = dP @ absv + SECOND * terms * (U if mode == 'f32' else 2 * U) * PV                       # apply_sum
    if mode == 'f16x2':
        bound = bound + SPLIT_REL * PV
    return ref, bound


def relation_grouped_statement(q, k, v, scale, groups, mode, grouped_apply=False, mistake=None):
    """hvr_relation_fwd_grouped: group g's rows of q [G Mq, D] against group g's rows of k / v [G Mk, D].
    mistake 'group_offset': every group but the first reads its K / V one row late."""
    G = int(groups)
    Mq, Mk = q.shape[0] // G, k.shape[0] // G
    refs, bounds = [], []
    for g in range(G):
        o = 1 if (mistake == 'group_offset' and g > 0) else 0
        rows = torch.arange(g * Mk + o, (g + 1) * Mk + o, device=k.device).clamp(max=k.shape[0] - 1)
        r, b = relation_statement(q[g * Mq:(g + 1) * Mq], k[rows], v[rows], scale, mode, grouped_apply,
                                  mistake if mistake != 'group_offset' else None)
        refs.append(r)
        bounds.append(b)
    return torch.cat(refs), torch.cat(bounds)


# ------------------------------------------------------------------------------------------------ comparisons
def compare(got, lo, hi, ref):
    """-> (worst |got - ref| / (wider half of [lo, hi]), number of elements outside [lo, hi], flat index of the worst)."""
    g = got.double()
    half = torch.maximum(hi - ref, ref - lo).clamp(min=1e-300)
    ratio = torch.where(g == ref, torch.zeros_like(g), (g - ref).abs() / half)
    bad = (g < lo) | (g > hi) | ~torch.isfinite(g)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    worst = ratio.reshape(-1).argmax() if ratio.numel() else torch.zeros((), dtype=torch.long)
    return (float(ratio.reshape(-1)[worst]) if ratio.numel() else 0.0), int(bad.sum()), int(worst)


def emulate_store(ref, mode, guard_rows=64, mistake=None, out_f32=False):
    """What a kernel that evaluates the (possibly mistaken) statement `ref` [M, N] exactly leaves in a SENTINEL-filled buffer of
    M + guard_rows rows.  'rows_past_M': the rows of the last 64-row tile past M are written from the clamped row M - 1;
    'trunc_store': truncation instead of round to nearest even."""
    M, N = ref.shape
    buf = torch.full((M + guard_rows, N), SENTINEL, dtype=torch.float64, device=ref.device)
    if out_f32 or mode == 'f32':
        st = ref.float().double()
    else:
        st = truncate_stored(ref.float().double(), mode) if mistake == 'trunc_store' else round_stored(ref.float().double(), mode)
    buf[:M] = st
    if mistake == 'rows_past_M':
        past = min(guard_rows, -M % 64 if M % 64 else 0)
        buf[M:M + past] = st[M - 1]
    return buf


def guard_intact(buf, M):
    return bool((buf[M:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ operand families
def real_operands(shape_a, shape_w, mode, seed, device='cpu', relu_like=True):
    """Real-statistics operands as f32 true values: activations after a ReLU (half of them zero, the rest |N(0, 1)|), weights
    N(0, 1 / sqrt(K)) like a folded conv's; rounded to what the mode stores."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape_a, generator=g)
    if relu_like:
        a = a.clamp(min=0.0)
    K = shape_w[-1] if len(shape_w) == 2 else shape_w[1] * shape_w[2] * shape_w[3]
    w = torch.randn(shape_w, generator=g) / math.sqrt(K)
    return store_true(a, mode, 'act').to(device), store_true(w, mode, 'weight').to(device)


def store_true(t, mode, role='act'):
    """True f32 values t rounded to what `mode` stores (f64 result)."""
    if mode == 'f16x2':
        return split_round(t.double(), ACT_SCALE if role == 'act' else WEIGHT_SCALE)
    return t.to(STORE[mode]).double()


def _ints(shape, lo, hi, g, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g, device=g.device).double()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g, device=g.device) < density)
    return v


def exact_case(shape_a, shape_w, mode, seed, family='plain', K=None, wide_bits=13, device='cpu'):
    """Exact-sum operands: a (activations) and w (weights) as f64 true values, bias, resid; every value an integer multiple of
    q = 2^-4, every product a multiple of q^2.  family:
      'plain'     |integers| <= 15 (exact in bf16, half, split half and f32);
      'lo_act'    split half: activations of up to `wide_bits` bits (non-zero lo half), sparse so that the sums stay exact, weights of
                  <= 3 bits (hi only): lo lo = 0 and hi(w) lo(a) is the only cross term;
      'lo_weight' the roles swapped.
    The caller asserts exactness with assert_exact on the statement's mag.  -> dict(a, w, bias, q, g: the generator, for exact_resid)"""
    g = torch.Generator(device=device).manual_seed(seed)
    q = 2.0 ** -4
    K = K or (shape_w[-1] if len(shape_w) == 2 else shape_w[1] * shape_w[2] * shape_w[3])
    if family == 'plain':
        a, w = _ints(shape_a, -15, 15, g), _ints(shape_w, -15, 15, g)
    else:
        assert mode == 'f16x2'
        top = 2 ** wide_bits - 1
        dens = min(1.0, 2.0 ** 24 / (8.0 * K * top * 7))            # worst-case sum|a||w| of the expected non-zeros: an eighth of the limit
        wide = lambda shp: _ints(shp, -top, top, g, dens)
        small = lambda shp: _ints(shp, -7, 7, g)
        a, w = (wide(shape_a), small(shape_w)) if family == 'lo_act' else (small(shape_a), wide(shape_w))
    N = shape_w[0]
    bias = _ints((N,), -2 ** 10, 2 ** 10, g) * q * q * 2 ** 4
    return dict(a=a * q, w=w * q, bias=bias, q=q, g=g)


def exact_resid(shape, g, q=2.0 ** -4):
    """A residual for the exact family: integers of <= 7 bits x 2^4 q^2 (exact in every format, a multiple of q^2)."""
    return _ints(shape, -127, 127, g) * q * q * 2 ** 4


def assert_exact(a, w, mag, q, mode, ref=None, qw=None):
    """The two conditions of the exact family: every operand value an integer multiple of q that its format stores exactly, and
    mag <= 2^24 q^2 per output element (so every partial sum, in any order, is an f32 number).  Split half: the condition is on the
    stored parts, sum(|hi| + |lo|)|w| <= mag (1 + 2^-10)."""
    qw = q if qw is None else qw                                   # (the stem's weights have a quantum of their own: products are multiples of q qw)
    for t, role, qq in ((a, 'act', q), (w, 'weight', qw)):
        assert bool((t / qq == (t / qq).round()).all()), 'operand not a multiple of the quantum'
        assert bool((store_true(t.float(), mode, role) == t).all()) and bool((t.float().double() == t).all()), 'operand not exact in its format'
    lim = 2.0 ** 24 * q * qw / (1 + 2.0 ** -10 if mode == 'f16x2' else 1.0)
    assert float(mag.max()) <= lim, 'sum|x||w| + |bias| + |resid| = %g exceeds 2^24 q^2 = %g' % (float(mag.max()), lim)
    if ref is not None and mode != 'f32':
        rng = 65504.0 / ACT_SCALE if mode == 'f16x2' else (65504.0 if mode == 'f16' else 3e38)
        assert float(ref.abs().max()) < rng, 'result leaves the range of the stored format'


TAIL_NEXT_FAMILIES = ('plain', 'lo_act', 'lo_weight', 'hn_lo_weight')


def exact_tail_next_case(hs, ws, wns, mode, seed, family='plain', device='cpu'):
    """Exact-sum operands of y = relu(h W3^T + b + resid), hn = relu(RN(y) wn^T + bn) (identity form), both products exact:
      'plain'        |integers| <= 15 in h / W3, <= 3 in wn;
      'lo_act' / 'lo_weight' (split half): the FIRST product carries one cross term (exact_case); y then has up to 24 significant bits, its
                     stored form a non-zero lo half, so with wn = two entries of +-q per row (hi only) the second product is exact and
                     carries lo(y) hi(wn) alone;
      'hn_lo_weight' (split half): h in +-q, W3 in +-3 q, small bias / residual: |y| / q^2 < 2^11, so lo(y) = 0; wn = one 12-bit odd entry
                     per row (lo(wn) != 0): the second product carries hi(y) lo(wn) alone.
    The caller asserts assert_exact on the first product and sum|RN(y)||wn| + |bn| <= 2^24 q^3 on the second.
    -> dict(h, w, bias, resid, wn, bn, q)"""
    q = 2.0 ** -4
    Cout, Cn = ws[0], wns[0]
    if family == 'hn_lo_weight':
        assert mode == 'f16x2'
        g = torch.Generator(device=device).manual_seed(seed)
        h, w = _ints(hs, -1, 1, g) * q, _ints(ws, -3, 3, g) * q
        bias = _ints((Cout,), -255, 255, g) * q * q
        resid = _ints(tuple(hs[:3]) + (Cout,), -1023, 1023, g) * q * q
        assert ws[1] * 3 + 255 + 1023 < 2 ** 11
        mag = _ints((Cn,), 1024, 2047, g) * 2 + 1                                  # odd, 12 bits: the lowest bit lies in the lo half
        sign = _ints((Cn,), 0, 1, g) * 2 - 1
        col = _ints((Cn,), 0, Cout - 1, g).long()
        wn = torch.zeros(wns, dtype=torch.float64, device=device)
        wn[torch.arange(Cn, device=device), col] = mag * sign * q
    else:
        c = exact_case(hs, ws, mode, seed, family=family, device=device)
        g, h, w, bias = c['g'], c['a'], c['w'], c['bias']
        resid = exact_resid(tuple(hs[:3]) + (Cout,), g)
        if family == 'plain':
            wn = _ints(wns, -3, 3, g) * q
        else:
            wn = torch.zeros(wns, dtype=torch.float64, device=device)
            for _ in range(2):
                col = _ints((Cn,), 0, Cout - 1, g).long()
                wn[torch.arange(Cn, device=device), col] = (_ints((Cn,), 0, 1, g) * 2 - 1) * q
    bn = _ints((Cn,), -64, 64, g) * q ** 3 * 2 ** 8
    return dict(h=h, w=w, bias=bias, resid=resid, wn=wn, bn=bn, q=q)


STEM_QW = 2.0 ** -10            # quantum of the wide stem weights: the kernel keeps them x 2^10 in half, so 13-bit integers x 2^-10 fit


def exact_stem_case(shape, mode, seed, family='plain', device='cpu'):
    """Exact-sum operands of the fused stem: img [B, 3, H, W], w [64, 7, 7, 3], bias [64].  'plain': |integers| <= 15 x q in both;
    'lo_act' (split half): an image of up to 13-bit integers x q (the kernel splits the unscaled image into hi + lo), sparse, weights
    of <= 3 bits; 'lo_weight': image of <= 3 bits, weights of up to 13-bit integers x STEM_QW (stem_split_weights keeps w x 2^10 in
    half: 8191 x 2^-10 x 2^10 fits), sparse.  Products are multiples of q qw.  -> dict(img, w, bias, q, qw)"""
    g = torch.Generator(device=device).manual_seed(seed)
    q = 2.0 ** -4
    qw = q
    K = 147
    top = 2 ** 13 - 1
    dens = min(1.0, 2.0 ** 24 / (8.0 * K * top * 7))
    if family == 'plain':
        img, w = _ints(shape, -15, 15, g) * q, _ints((64, 7, 7, 3), -15, 15, g) * q
    elif family == 'lo_act':
        assert mode == 'f16x2'
        img, w = _ints(shape, -top, top, g, dens) * q, _ints((64, 7, 7, 3), -7, 7, g) * q
    else:
        assert mode == 'f16x2' and family == 'lo_weight'
        qw = STEM_QW
        img, w = _ints(shape, -7, 7, g) * q, _ints((64, 7, 7, 3), -top, top, g, dens) * qw
    bias = _ints((64,), -1024, 1024, g) * q * qw * 16
    return dict(img=img, w=w, bias=bias, q=q, qw=qw)


def count_ties(ref, mode):
    """How many elements of the exact result lie on a rounding tie of the 16-bit format (truncation and round-half-up differ there)."""
    if mode in ('f32', 'f16x2'):
        return 0
    dt = STORE[mode]
    r = ref.float().to(dt)
    inf = torch.full_like(r, float('inf'))
    up, dn = torch.nextafter(r, inf).double(), torch.nextafter(r, -inf).double()
    rd = r.double()
    return int((((rd + up) / 2 == ref) | ((rd + dn) / 2 == ref)).sum())


# ------------------------------------------------------------------------------------------------ relation: the permutation family
LOG2E_F32 = 1.4426950408889634


def permutation_scale():
    """An f32 `scale` for which the kernel's logit factor fl(scale log2 e) is exactly 2^-5 -- whether the product is formed in f32 or
    in double and then rounded -- so that with dot products that are multiples of 32 every logit is an INTEGER in log2 units: block
    maxima, their integer roundings and every exp2 argument are exact, and P~ of a row's selected key is exp2(0) = 1."""
    s0 = torch.tensor(math.log(2.0) / 32.0, dtype=torch.float32)
    l32 = torch.tensor(LOG2E_F32, dtype=torch.float32)
    cand = s0
    for _ in range(8):
        cand = torch.nextafter(cand, torch.tensor(0.0))
    for _ in range(17):
        if float(cand * l32) == 2.0 ** -5 and float(torch.tensor(float(cand) * LOG2E_F32, dtype=torch.float64).float()) == 2.0 ** -5 \
                and float(torch.tensor(float(cand) * float(l32), dtype=torch.float64).float()) == 2.0 ** -5:
            return float(cand)
        cand = torch.nextafter(cand, torch.tensor(1.0))
    raise AssertionError('no f32 scale whose product with log2 e rounds to 2^-5')


PERM_C = 72.0                   # q / k amplitude: c^2 = 5184 = 162 x 32 -> one matching coordinate is worth 162 in log2 units
PERM_MARGIN_LOG2 = PERM_C * PERM_C / 32.0


def seams_crossed(sel, Mk):
    """True when every 128-key block boundary b (0 < b < Mk, b % 128 == 0) is straddled by some pair of ADJACENT query rows: one row
    selects a key below b and its neighbour a key at or above it -- so within one row tile the selected keys change block (and with
    them the 256-key score tile and the apply pass's K-step) at every seam of the key axis."""
    a, b = sel[:-1], sel[1:]
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    return all(bool(((lo < e) & (hi >= e)).any()) for e in range(128, Mk, 128))


def permutation_case(Mq, Mk, D, mode, seed, groups=1):
    """Query row i selects key sel[i]: keys are two-hot codes c (e_a + e_{D/2 + b}), (a, b) = (j mod D/2, j div D/2), queries carry the
    code of their key, so scale' q.k is 2 x 162 for the selected key and 162 or 0 for every other (log2 units, scale' = 2^-5 by
    permutation_scale).  f32's exp2 underflows to exactly 0 below 2^-149 (the smallest subnormal; half of it rounds to 0, and a
    hardware exponential that flushes subnormals gives 0 from 2^-126 down): the margin of 162 > 150 makes every other P~, and every
    block weight of a block without the selected key, exactly 0 -- asserted.  V: non-zero integers / 64 of <= 8 bits (exact in every
    format; non-zero so that nothing clamped below 2^-126 can surface in a sum).  sel runs over every 128-key block and, by its odd
    stride, over both sides of every 128 / 256 / 288 / 352-row seam.  -> q, k, v (f32 true values), sel"""
    assert PERM_MARGIN_LOG2 == 162.0 and PERM_MARGIN_LOG2 > 150.0        # 2^-162 < 2^-150 = half the smallest f32 subnormal -> 0
    assert D % 2 == 0 and Mk <= (D // 2) ** 2
    g = torch.Generator().manual_seed(seed)
    h = D // 2
    stride = max(1, Mk // max(Mq, 1)) | 1
    while math.gcd(stride, Mk) != 1:
        stride += 2
    qs, ks, vs, sels = [], [], [], []
    for grp in range(groups):
        sel = (torch.arange(Mq) * stride + 7 + 131 * grp) % Mk
        sel[0], sel[Mq - 1] = 0, Mk - 1                # a group's first and last key: what a K / V offset by one row loses or gains
        j = torch.arange(Mk)
        k = torch.zeros((Mk, D))
        k[j, j % h] = PERM_C
        k[j, h + j // h] = PERM_C
        q = k[sel].clone()
        v = torch.randint(1, 256, (Mk, D), generator=g).float() * (torch.randint(0, 2, (Mk, D), generator=g).float() * 2 - 1) / 64.0
        if Mq >= (Mk + 127) // 128:
            assert len(set((sel // 128).tolist())) == (Mk + 127) // 128, 'a 128-key block is never selected'
            assert seams_crossed(sel, Mk), 'a 128-key block boundary has no pair of adjacent rows selecting keys on its two sides'
        qs.append(q), ks.append(k), vs.append(v), sels.append(sel + grp * Mk)
    q, k, v = torch.cat(qs), torch.cat(ks), torch.cat(vs)
    for t in (q, k, v):
        assert bool((store_true(t, mode).float() == t).all())
    return q, k, v, torch.cat(sels)
