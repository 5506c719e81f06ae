"""f64 numpy statements of the global context block (include/hvr_hip.h, hvr_gcb_*) and of a Bottleneck that carries one
(mmdet/ops/context_block.py:64-104, mmdet/models/backbones/resnet.py:232-264), with error bounds counted from the rule's roundings.

The rule.  u [B,P,C] is one map, P = H * W pixels per frame, read in its stored format; everything below is per frame.
  pool       l[p] = sum_c u[p,c] wm[c] (+ the mask bias),  a = softmax_p(l),  ctx[c] = sum_p a[p] u[p,c]      ('avg': l = 0, a = 1/P)
  transform  h = W1 ctx + b1 (R = int(C ratio) rows),  g = relu(LN(h)) with the BIASED variance and eps = 1e-5 inside the root,
             o = W2 g + b2;  m = sigmoid(o_mul),  t = o_add
  apply      y = act(u m + t (+ resid)), the product first.
The mask bias shifts every logit of a frame alike, so a is the same with and without it (test_gcb_refs proves it on the statement);
the kernels do not take it.

The bounds (u32 = 2^-24; SECOND covers the second-order terms).  The device keeps f32 from the logits to m and t.
  logit      a dot product of C terms summed in f32 (per lane a chain of C / 64 terms, then six tree levels), whatever the order:
             |l^ - l| <= (C + K_DOT) u32 sum_c |u[p,c]| |wm[c]| =: dl[p].
  weights    the device forms exp(l^[p] - max^) with the running maximum subtracted: a logit error enters a weight RELATIVELY, by
             exp(+-dl).  Both the pixel's logit and the normaliser's carry one, the subtraction rounds once (u32 |l - max| <= u32 x the
             frame's logit range) and expf is good to 2 ulp = 4 u32: every a[p] is off by at most the factor
             w_rel = 2 max_p dl[p] + (range + K_EXP) u32.  Since sum_p a^ = 1 as well, ctx moves by at most 2 w_rel sum_p a[p] |u[p,c]|.
  ctx        the online sums: the pixels of a frame are cut into S runs (native.gcb_splits), a run keeps (max, sum, acc[C]), rescales when
             the maximum grows and adds one product per pixel; the S partials are rescaled against the frame maximum and added in a row;
             one division.  A rescale factor multiplies sum and acc alike and cancels in ctx = acc / sum, its own error with it.  What
             remains is the chain of additions and products: (P / S + S + K_CTX) u32 sum_p a[p] |u[p,c]|, the form the issue states.
             (Counted to the last rounding the worst case is P / S + 2 S + 9: numerator and denominator both walk the S partials.
             The tests hold the kernels to the tighter form; it is exceeded only if S > 7 AND every rounding falls the same way.)
  transform  dot products again: h errs by (C + K_DOT) u32 sum |W1| |ctx| + sum |W1| dctx =: D per row.  LayerNorm: the mean moves by at
             most D, the centred value by 2 D, sigma = sqrt(var + eps) by at most 2 D (d var <= 2 sqrt(var) 2 D, d sigma = d var / 2 sigma),
             so g moves by |gamma| (2 D / sigma + |h - mean| 2 D / sigma^2) plus (R + K_DOT) u32 (|g| + |beta|) for the two reductions and the
             affine.  o errs by sum |W2| dg + (R + K_DOT) u32 (sum |W2| |g| + |b2|); the sigmoid's slope is at most 1/4 and its evaluation
             (expf, add, divide) good to K_EXP u32.
             Link by link the tests are sharper than the chained bound: the pool is held to dctx on the f64 merge of the device's own
             partials (combine), the transform to its f32 bound on THAT context (combine_bound for the merge it does itself), the
             apply to its bound on the device's own m and t.  The chained bound is checked too, on the stored output.
  apply      u m + t + resid in f32: |u| dm + dt + 3 u32 (|u m| + |t| + |resid|), then ONE rounding into the stored format: half an
             ulp, which is at most the unit roundoff of the format times the value (bf16 2^-8, half 2^-11 and 2^-25 absolute for its
             subnormals, f32 u32; split half 2^-22 relative, 2^-24 / 16 absolute).
"""
import numpy as np

U32 = 2.0 ** -24
K_DOT = 8
K_EXP = 8
K_CTX = 16
SECOND = 1.05
EPS = 1e-5
STORE_REL = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11, 'f32': 2.0 ** -24, 'f16x2': 2.0 ** -22}
STORE_ABS = {'bf16': 0.0, 'f16': 2.0 ** -25, 'f32': 0.0, 'f16x2': 2.0 ** -28}
MODES = ('bf16', 'f16', 'f16x2', 'f32')
MISTAKES = ('softmax_channels', 'softmax_batch', 'no_max', 'ln_unbiased', 'ln_eps_outside', 'add_before_mul', 'no_sigmoid', 'after_residual',
            'before_bn3', 'round_planes', 'relu_inside')

# (B, H, W, C) of the kernel tests: one pixel; fewer pixels than a workgroup holds; several splits with a ragged last one; the widest map
SHAPES = ((1, 1, 1, 64), (2, 7, 9, 256), (3, 37, 53, 128), (1, 5, 3, 2048))
PLANES = (4, 16, 76)


def planes_of(C, ratio, mistake=None):
    """int() truncates (context_block.py:28); 'round_planes': round() instead."""
    return int(round(C * ratio)) if mistake == 'round_planes' else int(C * ratio)


def stored(x, mode):
    """f64 values -> the values a map of `mode` holds (RN; split half keeps hi + lo of the x 16 value)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    if mode == 'bf16':
        return t.float().to(torch.bfloat16).double().numpy()
    if mode == 'f16':
        return t.float().to(torch.float16).double().numpy()
    if mode == 'f16x2':
        s = t.float().double() * 16.0
        hi = s.to(torch.float16).double()
        return ((hi + (s - hi).to(torch.float16).double()) / 16.0).numpy()
    return t.float().double().numpy()


# ------------------------------------------------------------------------------------------------ the three steps
def pool_statement(u, wm=None, bm=0.0, mistake=None):
    """u [B,P,C] f64, wm [C] or None ('avg') -> dict(l [B,P], a [B,P], ctx [B,C]).  Mistakes: 'softmax_channels' nn.Softmax over the mask's
    ONE channel (every weight 1: ctx is the plain sum); 'softmax_batch' one softmax over the pixels of all frames; 'no_max' exp of the f32
    logits without the maximum subtracted."""
    B, P, C = u.shape
    if wm is None:
        l = np.zeros((B, P))
        a = np.full((B, P), 1.0 / P)
    else:
        l = u @ wm + bm
        if mistake == 'softmax_channels':
            a = np.ones((B, P))
        elif mistake == 'softmax_batch':
            e = np.exp(l - l.max())
            a = e / e.sum()
        elif mistake == 'no_max':
            with np.errstate(over='ignore', invalid='ignore'):
                e = np.exp(l.astype(np.float32))
                a = (e / e.sum(1, keepdims=True)).astype(np.float64)
        else:
            e = np.exp(l - l.max(1, keepdims=True))
            a = e / e.sum(1, keepdims=True)
    with np.errstate(invalid='ignore'):
        ctx = np.einsum('bp,bpc->bc', a, u)
    return dict(l=l, a=a, ctx=ctx)


def layer_norm(h, gamma, beta, mistake=None):
    R = h.shape[-1]
    mean = h.mean(-1, keepdims=True)
    d = h - mean
    var = (d * d).sum(-1, keepdims=True) / ((R - 1) if mistake == 'ln_unbiased' else R)
    sigma = (np.sqrt(var) + EPS) if mistake == 'ln_eps_outside' else np.sqrt(var + EPS)
    return d / sigma * gamma + beta, d, sigma


def branch_statement(ctx, br):
    """br = (w1 [R,C], b1 [R], gamma [R], beta [R], w2 [C,R], b2 [C]) -> (o [B,C], the intermediates for the bound)."""
    return _branch(ctx, br, None)[0]


def _branch(ctx, br, mistake):
    w1, b1, gamma, beta, w2, b2 = br
    h = ctx @ w1.T + b1
    n, d, sigma = layer_norm(h, gamma, beta, mistake)
    g = np.maximum(n, 0.0)
    return g @ w2.T + b2, dict(h=h, d=d, sigma=sigma, g=g)


def transform_statement(ctx, mul=None, add=None, mistake=None):
    """-> (m [B,C] or None, t [B,C] or None).  Mistakes: 'ln_unbiased', 'ln_eps_outside' (layer_norm), 'no_sigmoid' m = o_mul."""
    m = t = None
    if mul is not None:
        o = _branch(ctx, mul, mistake)[0]
        m = o if mistake == 'no_sigmoid' else 1.0 / (1.0 + np.exp(-o))
    if add is not None:
        t = _branch(ctx, add, mistake)[0]
    return m, t


def apply_statement(u, m=None, t=None, resid=None, relu=False, mistake=None):
    """u [B,P,C] -> act(u m + t (+ resid)).  'add_before_mul': (u + t) m; 'relu_inside': a ReLU on the block's output in front of the residual."""
    y = u
    if mistake == 'add_before_mul':
        y = (y + t[:, None, :]) if t is not None else y
        y = (y * m[:, None, :]) if m is not None else y
    else:
        y = (y * m[:, None, :]) if m is not None else y
        y = (y + t[:, None, :]) if t is not None else y
    if mistake == 'relu_inside':
        y = np.maximum(y, 0.0)
    if resid is not None:
        y = y + resid
    return np.maximum(y, 0.0) if relu else y


def context_statement(u, prm, resid=None, relu=False, mistake=None):
    """The whole block.  prm: dict(wm, bm, mul, add) (absent keys: None / 0).  -> dict(l, a, ctx, m, t, y)."""
    r = pool_statement(u, prm.get('wm'), prm.get('bm', 0.0), mistake)
    r['m'], r['t'] = transform_statement(r['ctx'], prm.get('mul'), prm.get('add'), mistake)
    r['y'] = apply_statement(u, r['m'], r['t'], resid, relu, mistake)
    return r


# ------------------------------------------------------------------------------------------------ the bounds
def splits(B, P):
    """hvr_gcb_splits (csrc/gcb.hip, gcb_split): at least 64 pixels per run, about 1024 runs per call, at most 256 per frame, none empty."""
    s = max(1, min((P + 63) // 64, max(1024 // B, 1), 256))
    chunk = -(-P // s)
    return -(-P // chunk), chunk


def pool_bound(u, wm, r):
    """-> dctx [B,C] for the pool of u with the statement's r = pool_statement(u, wm)."""
    B, P, C = u.shape
    S, chunk = splits(B, P)
    A = np.einsum('bp,bpc->bc', r['a'], np.abs(u))
    if wm is None:
        w_rel = 0.0
    else:
        dl = (C + K_DOT) * U32 * (np.abs(u) @ np.abs(wm))
        rng = r['l'].max(1) - r['l'].min(1)
        w_rel = (2.0 * dl.max(1) + (rng + K_EXP) * U32)[:, None]
    return SECOND * (2.0 * w_rel + (chunk + S + K_CTX) * U32) * A


def branch_bound(ctx, dctx, br):
    """-> do [B,C]: the error of W2 relu(LN(W1 ctx + b1)) + b2 for a context known to dctx."""
    w1, b1, gamma, beta, w2, b2 = br
    R, C = w1.shape
    _, it = _branch(ctx, br, None)
    D = ((C + K_DOT) * U32 * (np.abs(ctx) @ np.abs(w1).T + np.abs(b1)) + dctx @ np.abs(w1).T).max(-1, keepdims=True)
    dg = np.abs(gamma) * (2.0 * D / it['sigma'] + np.abs(it['d']) * 2.0 * D / it['sigma'] ** 2) + (R + K_DOT) * U32 * (it['g'] + np.abs(beta))
    return SECOND * (dg @ np.abs(w2).T + (R + K_DOT) * U32 * (it['g'] @ np.abs(w2).T + np.abs(b2)))


def transform_bound(ctx, dctx, mul=None, add=None):
    """-> (dm, dt), None for an absent branch."""
    dm = 0.25 * branch_bound(ctx, dctx, mul) + K_EXP * U32 if mul is not None else None
    dt = branch_bound(ctx, dctx, add) if add is not None else None
    return dm, dt


def combine(part):
    """The S partials [B,S,C+4] of a pool call (max, sum, 0, 0, acc[C]) as f64 -> (ctx [B,C], sum_j |acc_j| scale_j / den [B,C]): what the
    transform's first step computes, without its roundings."""
    part = np.asarray(part, dtype=np.float64)
    sc = np.exp(part[:, :, 0] - part[:, :, 0].max(1, keepdims=True))
    den = (part[:, :, 1] * sc).sum(1)[:, None]
    return (part[:, :, 4:] * sc[:, :, None]).sum(1) / den, (np.abs(part[:, :, 4:]) * sc[:, :, None]).sum(1) / den


def combine_bound(part):
    """The f32 merge of S partials: S products and S additions in numerator and denominator, S exps, one division."""
    S = np.asarray(part).shape[1]
    return SECOND * (2 * S + K_EXP + K_CTX) * U32 * combine(part)[1]


def store_bound(ref, b, mode):
    """b on the f32 value -> the bound on the stored value: half an ulp of the format on top."""
    return b + STORE_REL[mode] * (np.abs(ref) + b) + STORE_ABS[mode]


def apply_bound(u, m, t, resid, dm, dt, mode, y):
    """-> the bound on the stored y = act(u m + t (+ resid)) when m and t are known to dm and dt (None: exact)."""
    mag = np.abs(u * (m[:, None, :] if m is not None else 1.0)) + (np.abs(t)[:, None, :] if t is not None else 0.0) + (np.abs(resid) if resid is not None else 0.0)
    b = 3.0 * U32 * mag
    if dm is not None:
        b = b + np.abs(u) * dm[:, None, :]
    if dt is not None:
        b = b + dt[:, None, :]
    return store_bound(y, SECOND * b, mode)


def context_bound(u, prm, resid, mode, r):
    """The bound on the stored output of the whole block, r = context_statement(u, prm, resid, relu)."""
    dctx = pool_bound(u, prm.get('wm'), r)
    dm, dt = transform_bound(r['ctx'], dctx, prm.get('mul'), prm.get('add'))
    return apply_bound(u, r['m'], r['t'], resid, dm, dt, mode, r['y'])


def outside(got, ref, bound):
    """Number of elements of got outside ref +- bound (a non-finite element counts)."""
    with np.errstate(invalid='ignore'):
        return int((~(np.abs(got - ref) <= bound)).sum())


# ------------------------------------------------------------------------------------------------ inputs
def branch_params(g, C, R, w1_scale=1.0):
    """A branch with a randomised LAST conv (the reference zeroes it, which would make every numeric test vacuous)."""
    f = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731  (every parameter is an f32 value: the device holds the same numbers)
    return (f(g.standard_normal((R, C)) * w1_scale / np.sqrt(C)), f(g.standard_normal(R) * 0.1 * w1_scale), f(g.uniform(0.5, 1.5, R)),
            f(g.standard_normal(R) * 0.2), f(g.standard_normal((C, R)) / np.sqrt(R)), f(g.standard_normal(C) * 0.1))


def real_case(shape, mode, seed, pooling='att', fusion=('channel_add', 'channel_mul'), R=16, with_resid=True, w1_scale=1.0):
    """Stored-format inputs of one call: dict(u [B,P,C], resid, prm) with unit-scale maps and logits of a few units."""
    B, H, W, C = shape
    g = np.random.default_rng(seed)
    u = stored(g.standard_normal((B, H * W, C)), mode)
    resid = stored(g.standard_normal((B, H * W, C)), mode) if with_resid else None
    prm = dict(bm=0.0)
    if pooling == 'att':
        prm['wm'] = (g.standard_normal(C) * 2.0 / np.sqrt(C)).astype(np.float32).astype(np.float64)
    prm['mul'] = branch_params(g, C, R, w1_scale) if 'channel_mul' in fusion else None
    prm['add'] = branch_params(g, C, R, w1_scale) if 'channel_add' in fusion else None
    return dict(u=u, resid=resid, prm=prm, shape=shape)


def overflow_case(shape, mode, seed, peak='first'):
    """The overflow family: channel 0 of every pixel carries the logit (wm[0] = 1, the other mask weights tiny), drawn over about +-100, so
    that exp of the largest f32 logit is inf without the maximum subtracted.  peak: the run ('first' / 'last') that holds the frame
    maximum (+100); the pixels of the run at the other end sit at -100 and below, 200 under it: their weights underflow to exactly 0 in
    f32 (exp(-200) < 2^-149)."""
    B, H, W, C = shape
    P = H * W
    S, chunk = splits(B, P)
    assert S >= 3, 'the family needs a first, a middle and a last run'
    g = np.random.default_rng(seed)
    u = g.standard_normal((B, P, C))
    logit = g.uniform(-60.0, 60.0, (B, P))
    hi, lo = (slice(0, chunk), slice((S - 1) * chunk, P)) if peak == 'first' else (slice((S - 1) * chunk, P), slice(0, chunk))
    logit[:, lo] = g.uniform(-110.0, -100.0, logit[:, lo].shape)
    logit[:, hi] = g.uniform(80.0, 90.0, logit[:, hi].shape)
    logit[:, hi.start + 3] = 100.0
    u[:, :, 0] = logit
    u = stored(u, mode)
    wm = (g.standard_normal(C) * 1e-3).astype(np.float32).astype(np.float64)
    wm[0] = 1.0
    prm = dict(wm=wm, bm=0.0, mul=branch_params(g, C, 16), add=branch_params(g, C, 16))
    return dict(u=u, resid=stored(g.standard_normal((B, P, C)), mode), prm=prm, shape=shape, lo=lo, hi=hi)


# ------------------------------------------------------------------------------------------------ a Bottleneck with a context block
def conv_nhwc(x, w, stride=1, pad=0, dil=1, groups=1):
    """x [B,H,W,Cin], w [Cout,Cin/groups,KH,KW] (torch's layout) -> [B,OH,OW,Cout], f64."""
    B, H, W, Cin = x.shape
    Cout, Cg, KH, KW = w.shape
    OH, OW = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, OH, OW, Cout))
    og = Cout // groups
    for ky in range(KH):
        for kx in range(KW):
            tap = xp[:, ky * dil:ky * dil + (OH - 1) * stride + 1:stride, kx * dil:kx * dil + (OW - 1) * stride + 1:stride]
            for gi in range(groups):
                y[..., gi * og:(gi + 1) * og] += tap[..., gi * Cg:(gi + 1) * Cg] @ w[gi * og:(gi + 1) * og, :, ky, kx].T
    return y


def bn(x, sd, name):
    return (x - sd[name + '.running_mean']) / np.sqrt(sd[name + '.running_var'] + EPS) * sd[name + '.weight'] + sd[name + '.bias']


def block_params(sd, prefix='context_block.'):
    """The context block's parameters out of a state dict of f64 arrays (the reference's names)."""
    def branch(name):
        if prefix + name + '.0.weight' not in sd:
            return None
        w1 = sd[prefix + name + '.0.weight']
        R, C = w1.shape[:2]
        return (w1.reshape(R, C), sd[prefix + name + '.0.bias'], sd[prefix + name + '.1.weight'].reshape(R), sd[prefix + name + '.1.bias'].reshape(R),
                sd[prefix + name + '.3.weight'].reshape(C, R), sd[prefix + name + '.3.bias'])
    prm = dict(mul=branch('channel_mul_conv'), add=branch('channel_add_conv'), bm=0.0)
    if prefix + 'conv_mask.weight' in sd:
        prm['wm'] = sd[prefix + 'conv_mask.weight'].reshape(-1)
        prm['bm'] = float(sd[prefix + 'conv_mask.bias'].reshape(-1)[0])
    return prm


def bottleneck_statement(x, sd, stride=1, dil=1, groups=1, style='pytorch', mistake=None):
    """A Bottleneck with a context block (resnet.py:232-264) on x [B,H,W,Cin] from its state dict of f64 arrays -> [B,OH,OW,4 planes].
    Mistakes: 'after_residual' the block applied to out + identity; 'before_bn3' applied to conv3's output, bn3 behind it; 'relu_inside';
    and those of the three steps."""
    s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
    h = np.maximum(bn(conv_nhwc(x, sd['conv1.weight'], s1), sd, 'bn1'), 0.0)
    h = np.maximum(bn(conv_nhwc(h, sd['conv2.weight'], s2, dil, dil, groups), sd, 'bn2'), 0.0)
    out = conv_nhwc(h, sd['conv3.weight'])
    identity = bn(conv_nhwc(x, sd['downsample.0.weight'], stride), sd, 'downsample.1') if 'downsample.0.weight' in sd else x
    prm = block_params(sd)
    B, OH, OW, C = out.shape
    flat = lambda t: t.reshape(B, OH * OW, C)   # noqa: E731
    if mistake == 'before_bn3':
        y = bn(context_statement(flat(out), prm)['y'].reshape(out.shape), sd, 'bn3') + identity
    elif mistake == 'after_residual':
        y = context_statement(flat(bn(out, sd, 'bn3') + identity), prm)['y'].reshape(out.shape)
    else:
        y = context_statement(flat(bn(out, sd, 'bn3')), prm, flat(identity), False, mistake)['y'].reshape(out.shape)
    return np.maximum(y, 0.0)


def block_bound_f32(scale_of_output):
    """Bound on |an f32 evaluation of a golden Bottleneck - the f64 fixture| from the formats alone (C <= 256, planes 16 .. 64, K <= 576):
    three chained convs, each erring by at most (K + 3) u32 sum|x||w| with sum|x||w| some tens of the output's scale (weights N(0, 1/K),
    BatchNorm gains of 0.5 .. 1.5 over sqrt(0.5 .. 1.5)); the context block's pool and transforms add dot products over C <= 256 and
    R <= 64 terms whose errors pass through gains of order one (the f32 bound of the steps above on unit-scale inputs is below 1e-4);
    the f32 rounding of the parameters adds u32 per factor: 3 x 579 x 6e-8 x 40 = 4.2e-3 of the output's largest value -- the form and
    the constants of res2_refs.block_bound_f32.  (A misplaced or misnormalised context block errs by a tenth of the scale or more.)"""
    return 4.2e-3 * scale_of_output
