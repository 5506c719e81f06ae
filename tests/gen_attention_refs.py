"""f64 numpy statements of the generalized attention block (include/hvr_hip.h, hvr_gen_attn_fwd; ops.GeneralizedAttention) and of a
Bottleneck that carries one (mmdet/models/plugins/generalized_attention.py:196-372, mmdet/models/backbones/resnet.py:220-264), physical
NHWC, with error bounds counted from the rule's roundings.

The rule.  x [B,H,W,C]; heads, d = C // heads, s = kv_stride, t = the four type bits; keys on the grid x[:, ::s, ::s] of Hk x Wk.
  split      channel c of a projection is head c // d, component c % d
  q, k, v    1x1 convs without bias: q on x, k and v on the key grid
  tables     omega_i = 1000^(4 i / F), i < F / 4;  emb(D) = [sin(D / omega), cos(D / omega)] (concatenated);
             Px[x, xk] = fc_x(emb(mag (x - s xk))) / sqrt(2),  Py[y, yk] likewise with fc_y;  Gx = geom_bias . Px,  Gy = geom_bias . Py
  energy     E[p, j] = t0 q.k + t2 appr_bias.k + t1 (q.Px[x, xk] + q.Py[y, yk]) + t3 (Gx[x, xk] + Gy[y, yk]),   no 1 / sqrt(d)
  softmax    over the Hk Wk keys;  o = A v, heads concatenated;  y = gamma (proj_conv(o) + bias) + x.

The bounds (u32 = 2^-24, rel = the unit roundoff of the map's format: STORE_REL; SECOND covers the second-order terms).
  energy     every term is a dot product over d accumulated in f32 (on the MFMA or as FMAs, in whatever order) and the terms are added
             in f32: |E^ - E| <= (d + K_DOT) u32 Eabs with Eabs the same sum on absolute values  =: dE.
  weights    the device forms exp(E^ - m^) with the running maximum subtracted; a shift common to a query's keys cancels between
             numerator and normaliser, so an energy error enters a probability RELATIVELY, by exp(+-2 max_j dE).  The subtraction
             rounds once and the fast exp scales its argument by log2(e) first: (2 (m - E) + K_EXP) u32 relative, with m - E at most the
             query's energy range.  The kernel route then rounds the probability ONCE into the operand type of the second MFMA (rel;
             the composite keeps f32: u32) and sums exactly those rounded values into the normaliser.  (Half has a narrow exponent: a
             probability under 2^-14 is rounded absolutely, by at most 2^-25, against a normaliser that holds the maximum's 1:
             2^-25 sum_j |v_j - o| on top.)
             rho = expm1(2 max_j dE + (2 range + K_EXP) u32) + p_round.
  output     with weights w_j = a_j (1 + rho_j) / sum_i a_i (1 + rho_i), |rho_j| <= rho:  o^ - o = sum_j a_j rho_j (v_j - o) / (1 + sum a rho),
             at most rho / (1 - rho) sum_j a_j |v_j - o| -- zero for a v that is constant over the keys, whatever the energies.
             Numerator and normaliser are f32 chains over the Mk keys (16 per MFMA, in an order the hardware chooses) with one rescale
             per key block: 2 (Mk + 2 nblocks + K_ACC) u32 sum_j a_j |v_j|.  One division, ONE rounding into the format (store_bound).
  block      the projections are convs with f32 accumulation over C terms, rounded once into the format: dt = (C + K_DOT) u32 |x| |w| + rel |t|;
             the tables are rounded once into the format (rel |Px|), Gx / Gy and appr_bias into f32.  The energy is multilinear, so
             these move it by at most Eabs(|.| + d.) - Eabs(|.|), which joins dE above; dv joins as sum_j a_j dv_j (1 + rho).  The close
             is a conv over heads * d terms with the weight gamma W rounded into the format: |gamma| (do |W| + rel (|o| + do) |W|) +
             (Cq + K_DOT) u32 (|o| |gamma W| + |gamma b|), the residual add in its epilogue (3 u32), one rounding.
"""
import numpy as np

from tests import gcb_refs as G
from tests.gcb_refs import MODES, STORE_ABS, STORE_REL, U32, outside, store_bound, stored  # noqa: F401

K_DOT = 8
K_EXP = 8
K_ACC = 16
SECOND = 1.05
TYPES = ('1000', '0010', '0001', '1010', '1001', '0011', '1011', '0101', '0111', '1101', '1111')
REFUSED_TYPES = ('0100', '0110', '1100', '1110')
MISTAKES = ('scaled', 'heads_interleaved', 'kv_offset', 'kv_avg', 'px_by_y', 'sign_flipped', 'sincos_interleaved', 'no_sqrt2', 'geom_bias_dropped',
            'appr_bias_on_key', 'softmax_queries', 'gamma_on_residual', 'no_max')
# the statement against a fixture: u64 / u32 = 2^-29 = 1.9e-9 were the sums taken in the same order; another order changes which partial
# sums round, by at most the count of terms (<= 576 here): 1e-6 of the fixture's own f32 - f64 distance
FIXTURE_FACTOR = 1e-6


def bits(attention_type):
    return tuple(bool(int(c)) for c in attention_type)


# ------------------------------------------------------------------------------------------------ the links
def kv_grid(x, s, mistake=None):
    """x [B,H,W,C] -> the key / value map x[:, ::s, ::s].  'kv_offset': the grid starts at pixel 1; 'kv_avg': 2x2 means instead of samples."""
    B, H, W, C = x.shape
    ys, xs = np.arange(0, H, s), np.arange(0, W, s)
    if mistake == 'kv_offset':
        ys, xs = np.minimum(ys + 1, H - 1), np.minimum(xs + 1, W - 1)
    if mistake == 'kv_avg':
        y1, x1 = np.minimum(ys + 1, H - 1), np.minimum(xs + 1, W - 1)
        return 0.25 * (x[:, ys][:, :, xs] + x[:, y1][:, :, xs] + x[:, ys][:, :, x1] + x[:, y1][:, :, x1])
    return x[:, ys][:, :, xs]


def split_heads(t, heads, mistake=None):
    """[..., heads * d] -> [..., heads, d]: channel c is head c // d.  'heads_interleaved': head c % heads."""
    d = t.shape[-1] // heads
    if mistake == 'heads_interleaved':
        return np.swapaxes(t.reshape(t.shape[:-1] + (d, heads)), -1, -2)
    return t.reshape(t.shape[:-1] + (heads, d))


def merge_heads(o, mistake=None):
    if mistake == 'heads_interleaved':
        o = np.swapaxes(o, -1, -2)
    return o.reshape(o.shape[:-2] + (-1,))


def embedding(delta, F, mistake=None):
    omega = 1000.0 ** ((4.0 / F) * np.arange(0, F / 4))
    ang = delta[..., None] / omega
    if mistake == 'sincos_interleaved':
        return np.stack([np.sin(ang), np.cos(ang)], -1).reshape(delta.shape + (-1,))
    return np.concatenate([np.sin(ang), np.cos(ang)], -1)


def position_tables(prm, H, W, mistake=None):
    """-> (px [heads,W,Wk,d], py [heads,H,Hk,d]).  'sign_flipped': the difference key - query; 'no_sqrt2'; 'sincos_interleaved'."""
    s, out = prm['s'], []
    for n, fc in ((W, prm['fx']), (H, prm['fy'])):
        nk = (n - 1) // s + 1
        delta = prm['mag'] * (np.arange(n, dtype=np.float64)[:, None] - s * np.arange(nk, dtype=np.float64)[None, :])
        if mistake == 'sign_flipped':
            delta = -delta
        tab = embedding(delta, prm['F'], mistake) @ fc.T
        if mistake != 'no_sqrt2':
            tab = tab / np.sqrt(2.0)
        out.append(np.transpose(split_heads(tab, prm['heads'], mistake), (2, 0, 1, 3)))
    return out[0], out[1]


def energies(q, k, H, W, Hk, Wk, ab=None, px=None, py=None, gx=None, gy=None, qk=True, mistake=None):
    """The energy sum on whatever arrays it is handed (the statement's, or absolute values for the bounds) -> [B,heads,H*W,Hk*Wk].
    q [B,H*W,heads,d] or None, k [B,Hk*Wk,heads,d] or None, ab [heads,d], px / py as position_tables, gx [heads,W,Wk], gy [heads,H,Hk].
    'px_by_y': the x table indexed by the query's row."""
    src = q if q is not None else k
    B, heads = (src.shape[0], src.shape[2]) if src is not None else (1, gx.shape[0])
    E = np.zeros((B, heads, H, W, Hk, Wk))
    if qk:
        E = E + np.einsum('bphd,bkhd->bhpk', q, k).reshape(B, heads, H, W, Hk, Wk)
    if ab is not None:
        E = E + np.einsum('hd,bkhd->bhk', ab, k).reshape(B, heads, 1, 1, Hk, Wk)
    if px is not None:
        q5 = q.reshape(B, H, W, heads, -1)
        if mistake == 'px_by_y':
            ex = np.einsum('byxhd,hykd->bhyxk', q5, px[:, np.arange(H) % W])
        else:
            ex = np.einsum('byxhd,hxkd->bhyxk', q5, px)
        E = E + ex[:, :, :, :, None, :] + np.einsum('byxhd,hykd->bhyxk', q5, py)[:, :, :, :, :, None]
    if gx is not None:
        E = E + gx[None, :, None, :, None, :] + gy[None, :, :, None, :, None]
    return E.reshape(B, heads, H * W, Hk * Wk)


def core_statement(q, k, v, H, W, Hk, Wk, ab=None, px=None, py=None, gx=None, gy=None, qk=True, mistake=None):
    """The attention core on the operands the device is handed -> dict(E, A [B,heads,P,Mk], o [B,P,heads,d]).  'scaled': E / sqrt(d);
    'softmax_queries': the softmax over the query axis; 'no_max': exp of the f32 energies without the maximum subtracted."""
    E = energies(q, k, H, W, Hk, Wk, ab, px, py, gx, gy, qk, mistake)
    if E.shape[0] != v.shape[0]:
        E = np.broadcast_to(E, (v.shape[0],) + E.shape[1:])
    if mistake == 'scaled':
        E = E / np.sqrt(v.shape[-1])
    if mistake == 'no_max':
        with np.errstate(over='ignore', invalid='ignore'):
            e = np.exp(E.astype(np.float32))
            A = (e / e.sum(3, keepdims=True)).astype(np.float64)
    else:
        ax = 2 if mistake == 'softmax_queries' else 3
        e = np.exp(E - E.max(ax, keepdims=True))
        A = e / e.sum(ax, keepdims=True)
    with np.errstate(invalid='ignore'):
        o = np.einsum('bhpk,bkhd->bphd', A, v)
    return dict(E=E, A=A, o=o)


def core_bound(q, k, v, H, W, Hk, Wk, r, mode, ab=None, px=None, py=None, gx=None, gy=None, qk=True, p_round=None, key_block=64, dE_ops=0.0, dv=None):
    """The bound on the stored o [B,P,heads,d] of the core for r = core_statement(...) on the same operands.  p_round: the rounding of a
    probability (None: the format's, the kernel route; the composite: U32).  dE_ops / dv: what the operands' own errors add (block_bound)."""
    a = lambda t: None if t is None else np.abs(t)   # noqa: E731
    d, Mk = v.shape[-1], Hk * Wk
    dE = (d + K_DOT) * U32 * energies(a(q), a(k), H, W, Hk, Wk, a(ab), a(px), a(py), a(gx), a(gy), qk) + dE_ops
    E = r['E']
    rng = E.max(3) - E.min(3)
    rho = np.expm1(2.0 * dE.max(3) + (2.0 * rng + K_EXP) * U32) + (STORE_REL[mode] if p_round is None else p_round)      # [B,heads,P]
    rho = np.transpose(rho / (1.0 - np.minimum(rho, 0.5)), (0, 2, 1))[..., None]                                          # [B,P,heads,1]
    spread, flat = np.zeros_like(r['o']), np.zeros_like(r['o'])
    for p0 in range(0, r['o'].shape[1], 64):      # (in chunks of queries: the [P, Mk, heads, d] differences of a real map are GBs)
        sl = slice(p0, p0 + 64)
        dif = np.abs(v[:, None] - r['o'][:, sl, None])
        spread[:, sl], flat[:, sl] = np.einsum('bhpk,bpkhd->bphd', r['A'][:, :, sl], dif), dif.sum(2)
    mass = np.einsum('bhpk,bkhd->bphd', r['A'], np.abs(v))
    nb = -(-Mk // key_block)
    b = rho * spread + 2.0 * (Mk + 2 * nb + K_ACC) * U32 * mass
    if p_round is None:      # a probability below the format's normal range is rounded ABSOLUTELY (half: 2^-25), against a normaliser >= 1
        b = b + STORE_ABS[mode] * flat
    if dv is not None:
        b = b + (1.0 + rho) * np.einsum('bhpk,bkhd->bphd', r['A'], dv)
    return store_bound(r['o'], SECOND * b, mode)


# ------------------------------------------------------------------------------------------------ the block
def block_params(sd, cfg, prefix=''):
    """The block's parameters out of a state dict of f64 arrays (the reference's names) and its constructor keywords -> prm."""
    heads, t = cfg.get('num_heads', 9), bits(cfg.get('attention_type', '1111'))
    g = lambda n: sd.get(prefix + n)   # noqa: E731
    wv = g('value_conv.weight')
    Cq, C = wv.shape[:2]
    m = lambda w: None if w is None else w.reshape(w.shape[0], -1)   # noqa: E731
    F = cfg.get('position_embedding_dim', -1)
    return dict(heads=heads, d=Cq // heads, s=cfg.get('kv_stride', 2), t=t, F=F if F > 0 else C, mag=cfg.get('position_magnitude', 1),
                wq=m(g('query_conv.weight')), wk=m(g('key_conv.weight')), wv=m(wv), fx=g('appr_geom_fc_x.weight'), fy=g('appr_geom_fc_y.weight'),
                ab=g('appr_bias'), gb=g('geom_bias'), wo=m(g('proj_conv.weight')), bo=g('proj_conv.bias'), gamma=float(np.asarray(g('gamma')).reshape(-1)[0]))


def block_operands(x, prm, mode=None, mistake=None):
    """What the core is handed for x [B,H,W,C]: dict(q, k, v, ab, px, py, gx, gy, qk, H, W, Hk, Wk) with the '0010' type reduced to its one
    row (H = W = 1).  mode: the projections and the tables as a map of that format stores them (None: exact)."""
    t0, t1, t2, t3 = prm['t']
    heads, s = prm['heads'], prm['s']
    B, H, W, C = x.shape
    st = (lambda a: stored(a, mode)) if mode else (lambda a: a)   # noqa: E731
    xk = kv_grid(x, s, mistake)
    Hk, Wk = xk.shape[1:3]
    sp = lambda a: split_heads(a, heads, mistake)   # noqa: E731
    ops = dict(q=None, k=None, ab=None, px=None, py=None, gx=None, gy=None, qk=t0, H=H, W=W, Hk=Hk, Wk=Wk)
    if t0 or t1:
        ops['q'] = sp(st(x.reshape(B, H * W, C) @ prm['wq'].T))
    if t0 or t2:
        ops['k'] = sp(st(xk.reshape(B, Hk * Wk, C) @ prm['wk'].T))
    ops['v'] = sp(st(xk.reshape(B, Hk * Wk, C) @ prm['wv'].T))
    if t2:
        ops['ab'] = sp(prm['ab'])
    if t1 or t3:
        px, py = position_tables(prm, H, W, mistake)
        if t1:
            ops['px'], ops['py'] = st(px), st(py)
        if t3 and mistake != 'geom_bias_dropped':
            gb = sp(prm['gb'])[:, None, None, :]
            ops['gx'], ops['gy'] = (px * gb).sum(3), (py * gb).sum(3)
            if mode:
                ops['gx'], ops['gy'] = stored(ops['gx'], 'f32'), stored(ops['gy'], 'f32')
    if mistake == 'appr_bias_on_key' and t0 and t2:
        ops['k'], ops['ab'] = ops['k'] + ops['ab'][None, None], None       # q . (k + b) instead of (q + b) . k
    if not (t0 or t1 or t3):
        ops['H'] = ops['W'] = 1
    return ops


def core_of(ops, mistake=None):
    return core_statement(ops['q'], ops['k'], ops['v'], ops['H'], ops['W'], ops['Hk'], ops['Wk'], ops['ab'], ops['px'], ops['py'], ops['gx'], ops['gy'],
                          ops['qk'], mistake)


def close_statement(o, x, prm, mistake=None):
    """o [B,P or 1,heads,d] -> y = gamma (proj_conv(o) + bias) + x.  'gamma_on_residual': gamma (proj_conv(o) + bias + x)."""
    B, H, W, C = x.shape
    u = merge_heads(o, mistake) @ prm['wo'].T + prm['bo']
    u = np.broadcast_to(u, (B, H * W, C)).reshape(x.shape)
    return prm['gamma'] * (u + x) if mistake == 'gamma_on_residual' else prm['gamma'] * u + x


def block_statement(x, prm, mistake=None):
    """The whole block on x [B,H,W,C] -> dict(ops, E, A, o, y)."""
    ops = block_operands(x, prm, None, mistake)
    r = core_of(ops, mistake)
    r['ops'], r['y'] = ops, close_statement(r['o'], x, prm, mistake)
    return r


def block_bound(x, prm, mode, r, p_round=None, key_block=64):
    """The bound on the stored y of the whole block for r = block_statement(x, prm) (derivation: the module docstring, 'block')."""
    rel, ops = STORE_REL[mode], r['ops']
    B, H, W, C = x.shape
    heads = prm['heads']
    xk = kv_grid(x, prm['s'])
    a = lambda t: None if t is None else np.abs(t)   # noqa: E731

    def dproj(xx, w, t):
        n = xx.shape[0]
        return (C + K_DOT) * U32 * split_heads(np.abs(xx).reshape(n, -1, C) @ np.abs(w).T, heads) + rel * np.abs(t) + STORE_ABS[mode]
    dq = dproj(x, prm['wq'], ops['q']) if ops['q'] is not None else None
    dk = dproj(xk, prm['wk'], ops['k']) if ops['k'] is not None else None
    dv = dproj(xk, prm['wv'], ops['v'])
    up = lambda t, dt: None if t is None else np.abs(t) + dt   # noqa: E731
    args = (ops['H'], ops['W'], ops['Hk'], ops['Wk'])
    moved = energies(up(ops['q'], dq), up(ops['k'], dk), *args, a(ops['ab']), up(ops['px'], rel * a(ops['px'])) if ops['px'] is not None else None,
                     up(ops['py'], rel * a(ops['py'])) if ops['py'] is not None else None, up(ops['gx'], U32 * a(ops['gx'])) if ops['gx'] is not None else None,
                     up(ops['gy'], U32 * a(ops['gy'])) if ops['gy'] is not None else None, ops['qk'])
    base = energies(a(ops['q']), a(ops['k']), *args, a(ops['ab']), a(ops['px']), a(ops['py']), a(ops['gx']), a(ops['gy']), ops['qk'])
    do = core_bound(ops['q'], ops['k'], ops['v'], *args, r, mode, ops['ab'], ops['px'], ops['py'], ops['gx'], ops['gy'], ops['qk'], p_round, key_block,
                    dE_ops=moved - base, dv=dv)
    g, wo = abs(prm['gamma']), np.abs(prm['wo'])
    Cq = wo.shape[1]
    om, dom = merge_heads(np.abs(r['o'])), merge_heads(do)
    dy = g * (dom @ wo.T + rel * ((om + dom) @ wo.T)) + (Cq + K_DOT) * U32 * g * (om @ wo.T + np.abs(prm['bo']))
    dy = np.broadcast_to(dy, (B, H * W, C)).reshape(x.shape) + 3.0 * U32 * (np.abs(r['y']) + np.abs(x))
    return store_bound(r['y'], SECOND * dy, mode)


# ------------------------------------------------------------------------------------------------ a Bottleneck with an attention block
def bottleneck_statement(x, sd, cfg, stride=1, dil=1, style='pytorch', mistake=None):
    """A Bottleneck with a generalized attention block between relu(bn2(conv2)) and conv3 (resnet.py:220-264), and a context block behind
    bn3 where the state dict holds one, on x [B,H,W,Cin] from its state dict of f64 arrays -> [B,OH,OW,4 planes]."""
    s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
    h = np.maximum(G.bn(G.conv_nhwc(x, sd['conv1.weight'], s1), sd, 'bn1'), 0.0)
    h = np.maximum(G.bn(G.conv_nhwc(h, sd['conv2.weight'], s2, dil, dil), sd, 'bn2'), 0.0)
    h = block_statement(h, block_params(sd, cfg, 'gen_attention_block.'), mistake)['y']
    out = G.bn(G.conv_nhwc(h, sd['conv3.weight']), sd, 'bn3')
    identity = G.bn(G.conv_nhwc(x, sd['downsample.0.weight'], stride), sd, 'downsample.1') if 'downsample.0.weight' in sd else x
    if any(k.startswith('context_block.') for k in sd):
        B, OH, OW, C = out.shape
        out = G.context_statement(out.reshape(B, OH * OW, C), G.block_params(sd))['y'].reshape(out.shape)
    return np.maximum(out + identity, 0.0)


def bottleneck_bound_f32(scale_of_output):
    """Bound on |an f32 evaluation of a golden Bottleneck with an attention block - the f64 fixture| from the formats alone: the form and the
    constants of gcb_refs.block_bound_f32 (three chained convs erring by (K + 3) u32 sum|x||w|, K <= 576, sum|x||w| some tens of the output's
    scale) with a FOURTH link, the attention block: its projections and its close are convs over C <= 64 terms, and the projections' errors
    reach the output through the softmax with a gain of 2 sum|q||k| (a few units) on weights that sum to one -- 4 x 579 x 6e-8 x 40 = 5.6e-3
    of the output's largest value.  (A misplaced, mis-split or mis-indexed attention block errs by a tenth of the scale or more.)"""
    return 5.6e-3 * scale_of_output


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
def grid(query_tile, key_block):
    """(H, W, s) walking the kernel's tiles (native.gen_attn_tiles()): one key; fewer keys than a key block; exactly one block; one block
    plus one key; several blocks with a ragged tail; fewer queries than a query tile; W no multiple of the tile, so that a tile spans two
    image rows, with H != W; s = 3 with (H - 1) % s != 0."""
    kb, qt = key_block, query_tile
    assert kb % 8 == 0 and qt >= 16
    return ((1, 1, 1), (2, 2, 2), (3, 5, 1), (8, kb // 8, 1), (1, kb + 1, 1), (18, 2 * (kb // 4 + 1), 2), (20, 39, 3), (7, qt - 9, 2), (qt // 16 + 3, qt + 7, 3))


def core_case(B, heads, d, H, W, s, attention_type, mode, seed, energy_scale=1.0):
    """Stored-format operands of one core call (unit-scale v, energies of a few units): dict as block_operands gives it."""
    t0, t1, t2, t3 = bits(attention_type)
    g = np.random.default_rng(seed)
    Hk, Wk = (H - 1) // s + 1, (W - 1) // s + 1
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    n = lambda *shape: g.standard_normal(shape)   # noqa: E731
    sc = energy_scale * d ** -0.25
    ops = dict(q=None, k=None, ab=None, px=None, py=None, gx=None, gy=None, qk=t0, H=H, W=W, Hk=Hk, Wk=Wk)
    if t0 or t1:
        ops['q'] = stored(n(B, H * W, heads, d) * sc, mode)
    if t0 or t2:
        ops['k'] = stored(n(B, Hk * Wk, heads, d) * sc, mode)
    ops['v'] = stored(n(B, Hk * Wk, heads, d), mode)
    if t2:
        ops['ab'] = f32(n(heads, d) * sc)
    if t1:
        ops['px'], ops['py'] = stored(n(heads, W, Wk, d) * sc * 0.7, mode), stored(n(heads, H, Hk, d) * sc * 0.7, mode)
    if t3:
        ops['gx'], ops['gy'] = f32(n(heads, W, Wk) * energy_scale), f32(n(heads, H, Hk) * energy_scale)
    if not (t0 or t1 or t3):
        ops['H'] = ops['W'] = 1
    return ops
