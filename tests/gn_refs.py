"""f64 numpy statement of group normalisation as the kernels state it (include/hvr_hip.h, hvr_gn_*; torch.nn.GroupNorm with the
residual add and the ReLU of a Bottleneck's close), with error bounds counted from the rule's roundings.

The rule.  u [B,P,C] is one map, P = H * W pixels per frame, read in its stored format; G groups of Cg = C / G consecutive channels.
Per frame n and group g, over the N = P * Cg values of the group:
  mean = sum u / N,   var = sum (u - mean)^2 / N (biased),   rstd = 1 / sqrt(var + eps),   a[c] = rstd gamma[c]
  y = act((u - mean) a[c] + beta[c] (+ r)),   r = nothing | resid | (resid - mean_r) a_r[c] + beta_r[c]
the product first, then beta, then r, then the ReLU; one rounding into the stored format.

How the device gets there (the header): every value enters as v = u - K, K the group's pivot u[n][0][g Cg]; the frame's pixels are
cut into S = native.group_norm_splits(B, P, C) runs of chunk = ceil(P / S) pixels; a run is reduced by a workgroup of four waves, each
wave covering whole pixels, so a lane visits at most ceil(chunk / 4) pixels.  At every level the partial is centred, (n, mean - K, M2):
a 16-byte piece's values of one group (mean of at most 8 values, then the squared distances to it), the lane (one Chan merge per pixel it
visits), at most six xor-shuffle merges inside the wave, three merges across the waves, S - 1 across the runs.  The apply forms
c = (u - K) - (mean - K), then c a + beta (+ r).

The bounds (u32 = 2^-24, SECOND covers the second-order terms).  D = max |u - K| over the group; |mean - K| <= D and every difference
of two partial means is at most 2 D.
  levels   L = ceil(ceil(P / S) / 4) + S + K_TREE, K_TREE = 12: the Welford steps per lane, the S - 1 run merges, and six shuffle levels,
           three wave merges, the piece mean and the rounding of v with room to spare.  No term is measured on a device.
  mean     a merge computes ma + d wb with d = mb - ma (one rounding), wb = nb / n (the counts are exact integers, one rounding), the
           product and the sum (one each): it adds at most u32 (|m| + 4 |d wb|) <= 9 u32 D to the error it inherits, and what it inherits is a
           weighted mean of its operands' errors, at most the larger one.  The piece mean (up to 7 additions and one exact scaling of values
           of size D) stays inside the same 9 u32 D.  So  dm = 9 L u32 D.
  var      M2 is a sum of non-negative terms (qa + qb) + d^2 (na nb / n): per level at most 8 u32 relative (two roundings on d^2 and one
           inherited from d, three on the weight, the product, the sum).  A partial mean that is off by e changes d^2 w by 2 |d| |e| w to
           first order; over all merges sum |d| w <= sqrt(sum d^2 w  sum w) <= sqrt(M2  6 N) (Cauchy-Schwarz; the weights of a sequential
           chain -- lane steps, waves, runs -- sum to at most N each, those of a shuffle level to at most N / 2, six of them), with
           |e_b - e_a| <= 2 dm.  Rounding v = u - K moves every value by at most u32 D, the variance by at most 2 sqrt(var) u32 D.  So
             dvar = 8 L u32 var + (4 sqrt(6) dm + 2 u32 D) sqrt(var).
           (The piece's own M2 is taken around the piece's computed mean: an error there enters in second order only.)
  rstd     the division, the sum with eps, the root and the reciprocal are four roundings; rstd lies between 1 / sqrt(var + dvar + eps) and
           1 / sqrt(max(var - dvar, 0) + eps), widened by 4 u32.
  apply    five operations where the header's formula shows four (the pivot is subtracted on its own): c^ = ((u - K) - m^)
           errs by dc = dm + 3 u32 D; a^ = rstd^ gamma by da = |gamma| (drstd + u32 rstd); then the product, the sum with beta, the sum
           with r: dy = dc |a| + |c| da + 4 u32 (|c a| + |beta| + |r|) + dr, dr the same count on the normalised residual (0 for a plain one).
           The ReLU does not widen it.  ONE rounding into the stored format: forward_kernel_refs.stored_bracket.
A group of one repeated value has D = 0, var = 0, c = 0 exactly: y = RN(beta (+ r)) bit for bit, which test_gn_gpu asserts as an equality.
"""
import math

import numpy as np

U32 = 2.0 ** -24
K_TREE = 12
SECOND = 1.05
EPS = 1e-5
MISTAKES = ('sumsq', 'unbiased', 'eps_outside', 'group_interleaved', 'stats_across_frames', 'relu_before_resid', 'beta_before_scale',
            'resid_unnormalised', 'last_run_dropped', 'run_weights_equal')

# (B, H, W, C, G) of the kernel tests (the issue's table); RAGGED: the smallest map here with S >= 3 runs and a partly filled last one
GEOMETRIES = ((2, 5, 7, 64, 32), (3, 19, 23, 128, 32), (2, 9, 11, 256, 32), (2, 5, 7, 512, 32), (1, 6, 5, 1024, 32), (1, 6, 5, 2048, 32),
              (2, 5, 7, 128, 8), (2, 5, 7, 64, 1), (2, 1, 1, 64, 32), (1, 1, 3, 256, 32))
RAGGED = (1, 129, 131, 64, 32)


def splits(B, P, C=None):
    """hvr_gn_splits restated (test_gn_gpu asserts it equal to the library's): at least 64 pixels per run, about 1024 runs per call, at most 64
    per frame, no empty run -> (S, chunk)."""
    s = max(1, min((P + 63) // 64, max(1024 // B, 1), 64))
    chunk = -(-P // s)
    return -(-P // chunk), chunk


def levels(P, S):
    return -(-(-(-P // S)) // 4) + S + K_TREE


def _group_index(C, G, mistake):
    c = np.arange(C)
    return c % G if mistake == 'group_interleaved' else c // (C // G)


def _moments(u, G, eps, mistake, S):
    """u [B,P,C] f64 -> (mean, var, rstd) [B,C] (per channel, through its group) and D [B,C] = max |u - pivot| of the channel's group."""
    B, P, C = u.shape
    Cg = C // G
    gi = _group_index(C, G, mistake)
    mean, var, D = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    for g in range(G):
        sel = np.nonzero(gi == g)[0]
        x = u[:, :, sel]                                   # [B,P,Cg]
        if mistake == 'stats_across_frames':
            x = np.broadcast_to(x.reshape(1, B * P, Cg), (B, B * P, Cg))
        if mistake == 'last_run_dropped' and S > 1:
            x = x[:, :(S - 1) * -(-P // S)]
        N = x.shape[1] * Cg
        flat = x.reshape(B, N)
        if mistake == 'sumsq':                             # E[u^2] - E[u]^2, both sums accumulated in f32 in index order
            f = flat.astype(np.float32)
            m = np.cumsum(f, 1, dtype=np.float32)[:, -1] / np.float32(N)
            v = np.maximum(np.cumsum(f * f, 1, dtype=np.float32)[:, -1] / np.float32(N) - m * m, np.float32(0)).astype(np.float64)
            m = m.astype(np.float64)
        elif mistake == 'run_weights_equal' and S > 1:     # the runs' partials merged as if every run held as many values as the first
            chunk = -(-P // S)
            m, q, n = None, None, 0.0
            for s in range(S):
                xs = x[:, s * chunk:(s + 1) * chunk].reshape(B, -1)
                ms = xs.mean(1)
                qs = ((xs - ms[:, None]) ** 2).sum(1)
                nb = float(chunk * Cg)
                if m is None:
                    m, q, n = ms, qs, nb
                else:
                    d = ms - m
                    m, q, n = m + d * nb / (n + nb), q + qs + d * d * n * nb / (n + nb), n + nb
            v = q / n
        else:
            m = flat.mean(1)
            v = ((flat - m[:, None]) ** 2).sum(1) / ((N - 1) if mistake == 'unbiased' else N)
        mean[:, sel], var[:, sel] = m[:, None], v[:, None]
        D[:, sel] = np.abs(u[:, :, sel] - u[:, :1, sel[:1]]).max((1, 2))[:, None]
    rstd = 1.0 / (np.sqrt(var) + eps) if mistake == 'eps_outside' else 1.0 / np.sqrt(var + eps)
    return mean, var, rstd, D


def _norm_bound(u, gamma, beta, G, eps, S):
    """(the normalised map c a + beta, its error bound before any store, |c a|) of one map, all [B,P,C]."""
    B, P, C = u.shape
    mean, var, rstd, D = _moments(u, G, eps, None, S)
    L = levels(P, S)
    dm = 9.0 * L * U32 * D
    dvar = 8.0 * L * U32 * var + (4.0 * math.sqrt(6.0) * dm + 2.0 * U32 * D) * np.sqrt(var)
    hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    lo = 1.0 / np.sqrt(var + dvar + eps)
    drstd = np.maximum(hi - rstd, rstd - lo) + 4.0 * U32 * rstd
    c = u - mean[:, None, :]
    a = (rstd * gamma)[:, None, :]
    dc = (dm + 3.0 * U32 * D)[:, None, :]
    da = (np.abs(gamma) * (drstd + U32 * rstd))[:, None, :]
    val = c * a + beta
    return val, dc * np.abs(a) + np.abs(c) * da, np.abs(c * a)


def gn_statement(u, gamma, beta, G, eps=EPS, resid=None, resid_norm=None, relu=False, mistake=None, S=1):
    """u [B,P,C] f64 (the stored values), gamma / beta [C], resid like u or None, resid_norm = (gamma_r, beta_r) or None -> dict(y, bound):
    the rule by index arithmetic and the bound on the f32 value the device holds before its one store (module docstring).  S: the runs the
    device cuts a frame into (the bound's chain lengths; the mistakes 'last_run_dropped' and 'run_weights_equal').  A mistake returns y only."""
    assert mistake is None or mistake in MISTAKES, mistake
    B, P, C = u.shape
    mean, var, rstd, _ = _moments(u, G, eps, mistake, S)
    c = u - mean[:, None, :]
    a = (rstd * gamma)[:, None, :]
    val = (c + beta) * a if mistake == 'beta_before_scale' else c * a + beta
    r = None
    if resid is not None:
        r = resid
        if resid_norm is not None and mistake != 'resid_unnormalised':
            mr, vr, rr, _ = _moments(resid, G, eps, mistake, S)
            r = (resid - mr[:, None, :]) * (rr * resid_norm[0])[:, None, :] + resid_norm[1]
    if mistake == 'relu_before_resid':
        y = (np.maximum(val, 0.0) if relu else val) + (0.0 if r is None else r)
    else:
        y = val if r is None else val + r
        y = np.maximum(y, 0.0) if relu else y
    if mistake is not None:
        return dict(y=y)
    _, dy, ca = _norm_bound(u, gamma, beta, G, eps, S)
    mag = ca + np.abs(beta)
    if resid is not None:
        if resid_norm is not None:
            _, dr, car = _norm_bound(resid, resid_norm[0], resid_norm[1], G, eps, S)
            dy = dy + dr + 4.0 * U32 * (car + np.abs(resid_norm[1]))
        mag = mag + np.abs(r)
    return dict(y=y, bound=SECOND * (dy + 4.0 * U32 * mag))


# ------------------------------------------------------------------------------------------------ the rule in f32, on the CPU
F = np.float32


def _merge(na, ma, qa, nb, mb, qb):
    nt = na + nb
    with np.errstate(divide='ignore', invalid='ignore'):
        wb = np.where(nt > 0, nb / np.where(nt > 0, nt, F(1)), F(0)).astype(F)
    d = (mb - ma).astype(F)
    return nt, (ma + d * wb).astype(F), ((qa + qb) + (d * d).astype(F) * (na * wb).astype(F)).astype(F)


def _emulate_stats(x, G, eps, S, lanes):
    """x [B,P,C] -> (pivot, mean - pivot, rstd) [B,C] in f32 by the stated partial / merge rule: values relative to the pivot; per run `lanes`
    lanes, lane l visiting the pixels l, l + lanes, ... of the run, one centred partial per pixel and group merged into the lane's; the lanes
    by a pairwise tree (the lower lane first); the runs in order."""
    B, P, C = x.shape
    Cg = C // G
    xg = x.astype(F).reshape(B, P, G, Cg)
    piv = xg[:, 0, :, 0].copy()
    v = (xg - piv[:, None, :, None]).astype(F)
    chunk = -(-P // S)
    total = None
    for s in range(-(-P // chunk)):
        p0, p1 = s * chunk, min(P, (s + 1) * chunk)
        n, m, q = np.zeros((B, lanes, G), F), np.zeros((B, lanes, G), F), np.zeros((B, lanes, G), F)
        for t in range(-(-(p1 - p0) // lanes)):
            idx = p0 + t * lanes + np.arange(lanes)
            xx = v[:, np.minimum(idx, p1 - 1)]             # [B,lanes,G,Cg]
            sm = np.zeros((B, lanes, G), F)
            for e in range(Cg):
                sm = (sm + xx[..., e]).astype(F)
            mb = (sm * F(1.0 / Cg)).astype(F)
            qb = np.zeros((B, lanes, G), F)
            for e in range(Cg):
                dd = (xx[..., e] - mb).astype(F)
                qb = (qb + dd * dd).astype(F)
            nb = np.where(idx < p1, F(Cg), F(0)).astype(F)[None, :, None] * np.ones((B, lanes, G), F)
            qb = np.where(nb > 0, qb, F(0)).astype(F)       # (a lane past the run's end holds nothing)
            n, m, q = _merge(n, m, q, nb, mb, qb)
        w = lanes
        while w > 1:
            h = w // 2
            n, m, q = _merge(n[:, :h], m[:, :h], q[:, :h], n[:, h:w], m[:, h:w], q[:, h:w])
            w = h
        part = (n[:, 0], m[:, 0], q[:, 0])
        total = part if total is None else _merge(*total, *part)
    n, m, q = total
    rstd = (F(1) / np.sqrt((q / n).astype(F) + F(eps)).astype(F)).astype(F)
    rep = lambda t: np.repeat(t, Cg, axis=1)   # noqa: E731
    return rep(piv), rep(m), rep(rstd)


def emulate_f32(u, gamma, beta, G, eps=EPS, S=1, lanes=4, resid=None, resid_norm=None, relu=False):
    """The stated rule carried out in f32 on the CPU (lanes: a power of two) -> the f32 value before the store, as f64 [B,P,C]."""
    assert lanes & (lanes - 1) == 0
    k, m, rstd = _emulate_stats(u, G, eps, S, lanes)
    a = (rstd * gamma.astype(F)).astype(F)
    val = ((((u.astype(F) - k[:, None]).astype(F) - m[:, None]).astype(F) * a[:, None]).astype(F) + beta.astype(F)).astype(F)
    if resid is not None:
        r = resid.astype(F)
        if resid_norm is not None:
            kr, mr, rr = _emulate_stats(resid, G, eps, S, lanes)
            ar = (rr * resid_norm[0].astype(F)).astype(F)
            r = ((((r - kr[:, None]).astype(F) - mr[:, None]).astype(F) * ar[:, None]).astype(F) + resid_norm[1].astype(F)).astype(F)
        val = (val + r).astype(F)
    return (np.maximum(val, F(0)) if relu else val).astype(np.float64)


# ------------------------------------------------------------------------------------------------ operand families
def operands(family, mode, B, P, C, G, seed):
    """u [B,P,C] f64 on the grid of `mode` ('f32' / 'bf16' / 'f16').  real: conv-output statistics, zero mean, a per-channel scale spread
    over a decade; offset: a spread small against the mean (f32: 1000 + 0.01 N(0,1); bf16 / f16: the format's grid around 256 with unit-scale
    spread); constant: one repeated value per group and frame."""
    import torch
    g = np.random.default_rng(seed)
    if family == 'real':
        u = g.standard_normal((B, P, C)) * 10.0 ** g.uniform(-0.5, 0.5, C)
    elif family == 'offset':
        u = 1000.0 + 0.01 * g.standard_normal((B, P, C)) if mode == 'f32' else 256.0 + np.round(g.standard_normal((B, P, C))) * 2.0
    else:
        assert family == 'constant', family
        u = np.repeat(np.round(g.standard_normal((B, 1, G)) * 8.0) / 4.0, C // G, axis=2) * np.ones((1, P, 1))
    t = torch.from_numpy(u).float()
    t = t.to({'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[mode])
    return t.double().numpy()


def affine(C, seed):
    g = np.random.default_rng(seed)
    return (g.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64), (0.2 * g.standard_normal(C)).astype(np.float32).astype(np.float64))
