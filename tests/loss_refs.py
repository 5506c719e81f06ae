"""Plain float64 statements of the regression, IoU and GHM loss kernels (hvrnet_amd/csrc/reg_loss.hip, ghm.hip; the rules:
include/hvr_hip.h "Regression and IoU losses", "GHM losses"), written independently of the HIP code, with the error bounds that
tests/test_loss_refs.py (CPU) and tests/test_losses_gpu.py (GPU) hold the kernels to.

Error model and constants are those of tests/train_loss_refs.py (imported, not restated): u = 2^-24 per f32 operation, the library
functions' ulp limits, SECOND for the dropped products of errors, TINY per result that f32 rounds in its subnormal range.  A sum whose
longest chain of additions is c has error <= c u sum|term|.  No bound contains a value measured on a device.

Each rule is written ONCE, on the small arithmetic below, and evaluated twice:
  * on `Q` values: a float64 value v beside a bound e on |f32 result - v|.  Every operation of the rule adds its own rounding (u |v|
    for a sum or product, 2 DIV_ULP u |v| for a division, the library limits for logf / log1pf / expf / sqrtf) and carries its operands'
    bounds through by the operation's first-order slope.  This is the statement and its bound, counted from the rule's roundings.
  * on plain float32 tensors: the f32 emulation (the same text evaluated by PyTorch on the CPU at the kernels' precision).
A comparison (a branch of a rule, a max / min, a bin) is decided on the f64 values; the case generators keep every input away from the
places where f32 could decide otherwise (asserted there), except ties that compare two inputs directly, where the header's rule holds.
"""
import math

import torch

from tests.train_loss_refs import DIV_ULP, EXPF_ULP, LOG1PF_ULP, LOGF_ULP, SECOND, SQRTF_ULP, TINY, U, f32v
from tests.focal_refs import focal_loss_splits

MISTAKES = dict(
    balanced_l1=('branch_constant_dropped', 'log_base'),
    iou=('widths_without_plus_one', 'clamp_after_log'),
    bounded_iou=('eps_wrong_side',),
    ghmc=('right_closed_bins', 'tot_counts_invalid', 'weights_not_divided_by_n', 'momentum_updates_empty_bins', 'last_edge_at_one'),
    ghmr=('tot_as_count',))


# ------------------------------------------------------------------------------------------------ the arithmetic
class Q(object):
    """v: float64 value; e: bound on |the f32 result - v| (first order; the callers multiply by SECOND once at the end)."""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.v = self.v.double()
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x)

    def _r(self, v, e):           # one rounding of the result
        return Q(v, e + U * v.abs() + TINY * (v != 0).double())

    def __add__(self, o):
        o = Q.of(o)
        return self._r(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = Q.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Q.of(o) - self

    def __neg__(self):
        return Q(-self.v, self.e)

    def __mul__(self, o):
        o = Q.of(o)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Q.of(o)
        v = self.v / o.v
        den = (o.v.abs() - o.e).clamp(min=1e-300)
        return Q(v, (self.e + v.abs() * o.e) / den + 2 * DIV_ULP * U * v.abs() + TINY * (v != 0).double())

    def __rtruediv__(self, o):
        return Q.of(o) / self

    def abs(self):
        return Q(self.v.abs(), self.e)


def K(x, like):
    """A kernel argument (a C float) in the arithmetic of `like`."""
    return Q(f32v(x)) if isinstance(like, Q) else torch.tensor(f32v(x), dtype=torch.float32)


def half(x):    # exact in binary floating point
    return Q(x.v * 0.5, x.e * 0.5) if isinstance(x, Q) else x * 0.5


def twice(x):
    return Q(x.v * 2, x.e * 2) if isinstance(x, Q) else x * 2


def val(x):
    return x.v if isinstance(x, Q) else x.double()


def sel(c, a, b):
    if isinstance(a, Q) or isinstance(b, Q):
        a, b = Q.of(a), Q.of(b)
        return Q(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))      # (the side not taken may hold inf / nan: never mixed in)
    return torch.where(c, a, b)


def qmax(a, b):
    return sel(val(a) >= val(b), a, b)


def qmin(a, b):
    return sel(val(a) <= val(b), a, b)


def _lib(x, fn, slope_den, ulp):
    if isinstance(x, Q):
        v = fn(x.v)
        return Q(v, x.e / slope_den(x).clamp(min=1e-300) + 2 * ulp * U * v.abs() + TINY)
    return fn(x)


def qlog(x):
    return _lib(x, torch.log, lambda q: q.v.abs() - q.e, LOGF_ULP)


def qlog1p(x):
    return _lib(x, torch.log1p, lambda q: 1 + q.v - q.e, LOG1PF_ULP)


def qsqrt(x):
    return _lib(x, torch.sqrt, lambda q: 2 * torch.sqrt((q.v - q.e).clamp(min=1e-300)), SQRTF_ULP)


def qexp(x):
    if isinstance(x, Q):
        v = torch.exp(x.v)
        return Q(v, v * torch.expm1(x.e) + 2 * EXPF_ULP * U * v + TINY)
    return torch.exp(x)


def sign(x):
    return torch.sign(val(x)) if isinstance(x, Q) else torch.sign(x)


def lift(x, exact):
    """An input tensor in the arithmetic asked for: Q (exact f32 inputs taken as f64) or f32."""
    return Q(x.double()) if exact else x.float()


def zeros_like(x):
    return Q(torch.zeros_like(x.v)) if isinstance(x, Q) else torch.zeros_like(x)


def qsum(x, chain):
    """The sum of x over all elements by a reduction whose longest chain of additions is `chain`."""
    if isinstance(x, Q):
        return Q(x.v.sum(), x.e.sum() + chain * U * x.v.abs().sum())
    return x.sum()


def bound(q):
    return SECOND * q.e + TINY


def inside(got, q):
    """got (f32 or f64 tensor) lies inside the bound of the statement q."""
    return bool(((got.double().cpu() - q.v).abs() <= bound(q)).all())


# ------------------------------------------------------------------------------------------------ elementwise rules
def smooth_l1_rule(d, beta, like, mistake=None):
    a = d.abs()
    b = K(beta, like)
    inner = val(a) < val(b)
    l = sel(inner, half(a) * a / b, a - half(b))
    g = sel(inner, d / b, Q(sign(d)) if isinstance(d, Q) else sign(d))
    return l, g


def balanced_l1_rule(d, beta, alpha, gamma, like, mistake=None):
    a = d.abs()
    be, al, ga = K(beta, like), K(alpha, like), K(gamma, like)
    b64 = math.exp(f32v(gamma) / f32v(alpha)) - 1.0           # formed in f64 from the three floats; the kernel takes it rounded once
    b = Q(b64, torch.tensor(U * abs(b64), dtype=torch.float64)) if isinstance(like, Q) else K(b64, like)
    inner = val(a) < val(be)
    lg = qlog1p(b * a / be)
    if mistake == 'log_base':
        lg = lg * K(1.0 / math.log(10.0), like)
    li = al / b * (b * a + 1.0) * lg - al * a
    lo = ga * a if mistake == 'branch_constant_dropped' else ga * a + ga / b - al * be
    s = sign(d)
    s = Q(s) if isinstance(d, Q) else s
    return sel(inner, li, lo), sel(inner, (al * lg + al * ((1.0 - be) / (b * a + be))) * s, ga * s)


def mse_rule(d, like, mistake=None):
    return d * d, twice(d)


def reg_rule(rule, d, prm, like, mistake=None):
    if rule == 'smooth_l1':
        return smooth_l1_rule(d, prm['beta'], like)
    if rule == 'balanced_l1':
        return balanced_l1_rule(d, prm['beta'], prm['alpha'], prm['gamma'], like, mistake)
    assert rule == 'mse'
    return mse_rule(d, like)


def reg_elem(rule, pred, target, prm, exact=True, mistake=None):
    """'none' forms: (l, dl/dpred), [N, D] each, as Q (exact) or f32 tensors."""
    p, t = lift(pred, exact), lift(target, exact)
    return reg_rule(rule, p - t, prm, p, mistake)


def reduce_chain(N, D, ldp, wide_ok=True):
    """Longest chain of additions behind out1 of the elementwise family (focal_refs.focal_chain's count on D columns)."""
    S, rows = focal_loss_splits(N, D)
    steps = 0
    for V in ((1, 4) if (D % 4 == 0 and ldp % 4 == 0 and wide_ok) else (1,)):
        pieces = -(-D // V)
        G = min(256, pieces)
        R = 256 // G
        steps = max(steps, -(-rows // R) * -(-pieces // G) * V)
    return steps + 6 + 4 + -(-S // 64) + 6


def _reduced(l, g, w, loss_weight, avg, chain, like, expand=None):
    """out1 = (sum w l) * (loss_weight / avg), grad = (loss_weight / avg * w) g."""
    scale = K(loss_weight, like) / K(avg, like)
    wl = l if w is None else w * l
    out1 = qsum(wl, chain) * scale
    c = scale if w is None else scale * w
    if w is None:     # the kernel multiplies by w = 1: exact
        c = scale * (Q(torch.ones_like(l.v)) if isinstance(l, Q) else torch.ones_like(l))
    return out1, c


def reg_reduced(rule, pred, target, w, prm, loss_weight, avg, ldp=None, exact=True, mistake=None, chain=None):
    """hvr_reg_loss: -> (out1 0-dim, d_pred [N, D]).  chain: the longest chain of additions to count instead of the kernel's own (a caller that
    holds ANOTHER kernel's sum of the same terms to the statement passes the number of terms, which bounds every order)."""
    l, g = reg_elem(rule, pred, target, prm, exact, mistake)
    N, D = pred.shape
    wq = None if w is None else lift(w, exact)
    out1, c = _reduced(l, g, wq, loss_weight, avg, reduce_chain(N, D, ldp or D) if chain is None else chain, l)
    return out1, c * g


# ------------------------------------------------------------------------------------------------ box-pair rules
def iou_rule(p, t, eps, like, mistake=None):
    """p, t: lists of the four coordinate columns -> (l [n], g list of four [n])."""
    one = 0.0 if mistake == 'widths_without_plus_one' else 1.0
    lx, ly, rx, ry = qmax(p[0], t[0]), qmax(p[1], t[1]), qmin(p[2], t[2]), qmin(p[3], t[3])
    zero = zeros_like(p[0])
    w, h = qmax(rx - lx + one, zero), qmax(ry - ly + one, zero)
    I = w * h
    pw, ph = p[2] - p[0] + one, p[3] - p[1] + one
    a1, a2 = pw * ph, (t[2] - t[0] + one) * (t[3] - t[1] + one)
    Un = a1 + a2 - I
    iou = I / Un
    e = K(eps, like)
    live = val(iou) >= val(e)
    pv, tv = [val(x) for x in p], [val(x) for x in t]
    dI = [sel(pv[0] >= tv[0], -h, zero), sel(pv[1] >= tv[1], -w, zero), sel(pv[2] <= tv[2], h, zero), sel(pv[3] <= tv[3], w, zero)]
    dA = [-ph, -pw, ph, pw]
    g = [sel(live, (dA[k] - dI[k]) / Un - dI[k] / I, zero) for k in range(4)]
    if mistake == 'clamp_after_log':
        l = -qmax(qlog(iou), e + zero)
    else:
        l = -qlog(sel(live, iou, e + zero))
    return l, g


def _switch(c, beta):
    inner = val(c) < val(beta)
    one = (Q(torch.ones_like(c.v)) if isinstance(c, Q) else torch.ones_like(c))
    return sel(inner, half(c) * c / beta, c - half(beta)), sel(inner, c / beta, one)


def _bounded_axis(p1, p2, t1, t2, beta, eps, mistake):
    pc, tc = half(p1 + p2), half(t1 + t2)
    pw, tw = p2 - p1 + 1.0, t2 - t1 + 1.0
    dx = tc - pc
    a2 = twice(dx.abs())
    zero = zeros_like(p1)
    if mistake == 'eps_wrong_side':
        den = tw + a2
        f = (tw - a2 + eps) / den
        r1, r2 = (tw + eps) / pw, (pw + eps) / tw
    else:
        den = tw + a2 + eps
        f = (tw - a2) / den
        r1, r2 = tw / (pw + eps), pw / (tw + eps)
    cl, cs = _switch(1.0 - qmax(f, zero), beta)
    cg = sel(val(f) > 0, cs * (twice(twice(tw) + eps) / (den * den)) * -(Q(sign(dx)) if isinstance(dx, Q) else sign(dx)), zero)
    sl, ss = _switch(1.0 - qmin(r1, r2), beta)
    sg = sel(val(r1) <= val(r2), ss * (tw / ((pw + eps) * (pw + eps))), ss * (-1.0 / (tw + eps)))
    return (cl, cg), (sl, sg)


def bounded_iou_rule(p, t, beta, eps, like, mistake=None):
    """-> (l list of four [n] in the order dx, dy, dw, dh; their slopes with respect to (centre x, centre y, width, height))."""
    b, e = K(beta, like), K(eps, like)
    (cxl, cxg), (sxl, sxg) = _bounded_axis(p[0], p[2], t[0], t[2], b, e, mistake)
    (cyl, cyg), (syl, syg) = _bounded_axis(p[1], p[3], t[1], t[3], b, e, mistake)
    return [cxl, cyl, sxl, syl], [cxg, cyg, sxg, syg]


def _stack(cols):
    if isinstance(cols[0], Q):
        return Q(torch.stack([c.v for c in cols], 1), torch.stack([c.e for c in cols], 1))
    return torch.stack(cols, 1)


def _cols(x, exact):
    x = lift(x, exact)
    return [Q(x.v[:, k], x.e[:, k]) for k in range(4)] if exact else [x[:, k] for k in range(4)]


def box_chain(n, per_row):
    S, rows = focal_loss_splits(n, 4)
    return -(-rows // 256) * per_row + 6 + 4 + -(-S // 64) + 6


def box_forms(rule, pred, target, prm, exact=True, mistake=None, coef=None):
    """The box-pair family on pred, target [n, 4]: -> (l, d_pred) where l is [n] ('iou') / [n, 4] ('bounded_iou') and d_pred [n, 4] is
    the gradient of sum(coef * l) (coef in the loss's shape, Q / f32; None: ones) in the kernels' order of operations."""
    p, t = _cols(pred, exact), _cols(target, exact)
    if rule == 'iou':
        l, g = iou_rule(p, t, prm['eps'], p[0], mistake)
        if coef is None:
            coef = Q(torch.ones_like(l.v)) if exact else torch.ones_like(l)
        return l, _stack([coef * g[k] for k in range(4)])
    l, s = bounded_iou_rule(p, t, prm['beta'], prm['eps'], p[0], mistake)
    if coef is None:
        c = [Q(torch.ones_like(l[0].v)) if exact else torch.ones_like(l[0])] * 4
    else:
        c = [Q(coef.v[:, k], coef.e[:, k]) for k in range(4)] if exact else [coef[:, k] for k in range(4)]
    gcx, gcy, gsx, gsy = half(c[0] * s[0]), half(c[1] * s[1]), c[2] * s[2], c[3] * s[3]
    return _stack(l), _stack([gcx - gsx, gcy - gsy, gcx + gsx, gcy + gsy])


def box_reduced(rule, pred, target, w, prm, loss_weight, avg, exact=True, mistake=None):
    """hvr_box_loss: -> (out1 0-dim, d_pred [n, 4])."""
    n = pred.shape[0]
    l, _ = box_forms(rule, pred, target, prm, exact, mistake)
    like = l
    scale = K(loss_weight, like) / K(avg, like)
    if w is None:
        wq = Q(torch.ones_like(l.v)) if exact else torch.ones_like(l)
    else:
        wq = lift(w, exact)
    out1 = qsum(wq * l, box_chain(n, 1 if rule == 'iou' else 4)) * scale
    _, d = box_forms(rule, pred, target, prm, exact, mistake, coef=scale * wq)
    return out1, d


# ------------------------------------------------------------------------------------------------ GHM
def ghm_edges(bins, kind):
    """The modules' edges buffer in f32: i / bins with the last edge + 1e-6 (GHMC) or 1000 (GHMR)."""
    e = torch.arange(bins + 1).float() / bins
    if kind == 'ghmc':
        e[-1] += 1e-6
    else:
        e[-1] = 1e3
    return e


def ghm_splits(N, C):
    """hvr_ghm_splits restated: (S, elements per workgroup)."""
    S, _ = focal_loss_splits(N, C)
    E = N * C
    per = -(-E // S)
    return -(-E // per), per


def ghm_chain(N, C):
    S, per = ghm_splits(N, C)
    return -(-per // 256) + 6 + 4 + -(-S // 64) + 6


def expand_binary_labels(labels, label_weights, C):
    """_expand_binary_labels (ghm_loss.py:8-15): label k >= 1 marks column k - 1."""
    t = (labels[:, None] == torch.arange(1, C + 1)[None, :]).float()
    return t, label_weights[:, None].expand(-1, C).contiguous()


def _ghm_g(kind, pred, target, mu, exact):
    """(g, x or d, r) per element: GHMC r = sigmoid(x) in the stable forms; GHMR r = sqrt(d d + mu mu)."""
    p, t = lift(pred, exact), lift(target, exact)
    if kind == 'ghmc':
        ex = qexp(-p.abs())
        r = 1.0 / (1.0 + ex)
        sg = sel(val(p) >= 0, r, ex * r)
        return (sg - t).abs(), p, sg, t
    d = p - t
    m = K(mu, p)
    r = qsqrt(d * d + m * m)
    return (d / r).abs(), d, r, t


def ghm_statement(kind, pred, target, weight, edges, momentum=0.0, acc=None, loss_weight=1.0, mu=0.02, exact=True, mistake=None):
    """hvr_ghmc_loss / hvr_ghmr_loss on dense [N, C] inputs (weight [N, C]; the labels form is expanded by the caller) ->
    dict(counts int64 [bins], n int, tot, w [bins], acc [bins] or None, out1, d [N, C], g): Q values (exact) or f32 tensors."""
    N, C = pred.shape
    bins = edges.numel() - 1
    edges = edges.clone()
    if mistake == 'last_edge_at_one':
        edges[-1] = 1.0
    g, x, r, t = _ghm_g(kind, pred, target, mu, exact)
    gv, ed = val(g), edges.double()
    valid = weight > 0
    binidx = torch.full((N, C), -1, dtype=torch.long)
    counts = torch.zeros(bins, dtype=torch.long)
    for i in range(bins):
        inb = ((gv > ed[i]) & (gv <= ed[i + 1])) if mistake == 'right_closed_bins' else ((gv >= ed[i]) & (gv < ed[i + 1]))
        inb = inb & valid
        binidx[inb] = i
        counts[i] = int(inb.sum())
    like = g
    chain = ghm_chain(N, C)
    if kind == 'ghmc':
        cnt = float(N * C) if mistake == 'tot_counts_invalid' else float(valid.sum())
        tot = K(max(cnt, 1.0), like)          # an integer sum: exact
    else:
        if mistake == 'tot_as_count':
            tot = K(max(float(valid.sum()), 1.0), like)
        else:
            tot = qmax(qsum(lift(weight, exact), chain), K(1.0, like))
    n = int((counts > 0).sum())
    mom = K(momentum, like)
    cf = Q(counts.double()) if exact else counts.float()
    nonempty = counts > 0
    accq = None
    if momentum > 0:
        a0 = lift(acc, exact)
        upd = mom * a0 + (1.0 - mom) * cf
        accq = upd if mistake == 'momentum_updates_empty_bins' else sel(nonempty, upd, a0)
        denom = upd
    else:
        denom = cf
    safe = sel(nonempty, denom, (Q(torch.ones(bins, dtype=torch.float64)) if exact else torch.ones(bins)))
    nn_ = K(1.0 if mistake == 'weights_not_divided_by_n' else float(max(n, 1)), like)
    w = sel(nonempty, tot / safe / nn_, zeros_like(safe))
    # per-element bin weight
    inbin = binidx >= 0
    idx = binidx.clamp(min=0)
    wb = Q(w.v[idx], w.e[idx]) if exact else w[idx]
    zero = zeros_like(g)
    lw = K(loss_weight, like)
    if kind == 'ghmc':
        term = qmax(x, zero) - x * t + qlog1p(qexp(-x.abs()))
        slope = r - t
    else:
        term = r - K(mu, like)
        slope = x / r
    out1 = lw * qsum(sel(inbin, wb * term, zero), chain) / tot
    d = sel(inbin, lw * wb * slope / tot, zero)
    return dict(counts=counts, n=n, tot=tot, w=w, acc=accq, out1=out1, d=d, g=gv, bin=binidx)


# ------------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def reg_case(N, D, seed, beta=1.0, scale=1.5):
    """pred, target f32 [N, D] and weights [N, D] in [0.5, 1.5) with exact zeros on about a fifth (and on element 0 when there are two
    or more).  |pred - target| stays at least 1e-3 away from beta and from 0 (no element on a kink of a rule)."""
    g = _gen(seed)
    pred, target = torch.randn((N, D), generator=g) * scale, torch.randn((N, D), generator=g) * scale
    b32 = f32v(beta)
    for _ in range(8):
        d = (pred - target).double()
        near = ((d.abs() - b32).abs() < 2e-3) | (d.abs() < 2e-3)
        if not bool(near.any()):
            break
        target = torch.where(near, target + 0.0137, target)
    d = (pred - target).double()
    assert bool((((d.abs() - b32).abs() >= 1e-3) & (d.abs() >= 1e-3)).all())
    w = 0.5 + torch.rand((N, D), generator=g)
    w[torch.rand((N, D), generator=g) < 0.2] = 0.0
    if N * D >= 2:
        w.view(-1)[0] = 0.0
    return pred, target, w


BOX_KINDS = ('overlap', 'disjoint', 'nested', 'identical', 'degenerate')


def box_case(n, seed, beta=0.2, eps=1e-3, iou_eps=1e-6):
    """pred, target f32 [n, 4] on a quarter-pixel grid (every sum and difference of coordinates is exact in f32, so the comparisons of
    the rules see the same operands in f32 and f64), row i of kind BOX_KINDS[i % 5]: overlapping, disjoint (iou = 0), target nested
    in pred, identical (every max / min ties: the header's rule), pred degenerate (zero width: x2 = x1 - 1).  Asserted: no bounded-IoU
    term within 1e-3 of its switch at beta or of the zero of its max, no two ratios within 1e-4 unless equal, no iou within a factor 2
    of iou_eps.  -> (pred, target, w_row [n], w_elem [n, 4])."""
    g = _gen(seed)

    def grid(x):
        return torch.round(x * 4) / 4

    xy = grid(torch.rand((n, 2), generator=g) * 200)
    wh = grid(8 + torch.rand((n, 2), generator=g) * 80)
    target = torch.cat([xy, xy + wh], 1)
    pred = torch.empty_like(target)
    for i in range(n):
        k = BOX_KINDS[i % 5]
        t = target[i]
        w_, h_ = wh[i]
        if k == 'overlap':
            sh = grid((torch.rand(2, generator=g) - 0.5) * 0.6 * wh[i])
            sc = grid(wh[i] * (0.7 + 0.6 * torch.rand(2, generator=g)))
            pred[i] = torch.cat([xy[i] + sh, xy[i] + sh + sc])
        elif k == 'disjoint':
            off = torch.stack([w_ + 5.25, h_ + 3.5])
            pred[i] = torch.cat([xy[i] + off, xy[i] + off + wh[i]])
        elif k == 'nested':
            pred[i] = torch.stack([t[0] - 2.25, t[1] - 1.5, t[2] + 3.75, t[3] + 2.5])
        elif k == 'identical':
            pred[i] = t
        else:
            pred[i] = torch.stack([t[0] + 1.25, t[1] + 0.5, t[0] + 0.25, t[3] - 0.75])
    # move rows whose bounded-IoU terms sit near a switch
    for _ in range(12):
        bad = _box_near_switch(pred, target, beta, eps, iou_eps)
        if not bool(bad.any()):
            break
        pred = torch.where(bad[:, None], pred + torch.tensor([0.75, 0.5, 1.25, 1.0]), pred)
    assert not bool(_box_near_switch(pred, target, beta, eps, iou_eps).any())
    w_row = 0.5 + torch.rand(n, generator=g)
    w_row[torch.rand(n, generator=g) < 0.2] = 0.0
    w_elem = 0.5 + torch.rand((n, 4), generator=g)
    w_elem[torch.rand((n, 4), generator=g) < 0.2] = 0.0
    if n >= 2:
        w_row[0] = 0.0
        w_elem[0, 0] = 0.0
    return pred, target, w_row, w_elem


def _box_near_switch(pred, target, beta, eps, iou_eps):
    p, t = pred.double(), target.double()
    bad = torch.zeros(pred.shape[0], dtype=torch.bool)
    b, e = f32v(beta), f32v(eps)
    for a in (0, 1):
        pc, tc = (p[:, a] + p[:, a + 2]) / 2, (t[:, a] + t[:, a + 2]) / 2
        pw, tw = p[:, a + 2] - p[:, a] + 1, t[:, a + 2] - t[:, a] + 1
        a2 = 2 * (tc - pc).abs()
        f = (tw - a2) / (tw + a2 + e)
        r1, r2 = tw / (pw + e), pw / (tw + e)
        c1, c2 = 1 - f.clamp(min=0), 1 - torch.min(r1, r2)
        bad |= ((c1 - b).abs() < 1e-3) | ((c2 - b).abs() < 1e-3) | (f.abs() < 1e-3) | (((r1 - r2).abs() < 1e-4) & (pw != tw))
    lt, rb = torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])
    whi = (rb - lt + 1).clamp(min=0)
    I = whi[:, 0] * whi[:, 1]
    Un = (p[:, 2] - p[:, 0] + 1) * (p[:, 3] - p[:, 1] + 1) + (t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1) - I
    iou = I / Un
    bad |= (iou > 0) & (iou < 2 * iou_eps)
    return bad


GHM_MARGIN = 1e-5


def _near_edge(g, edges):
    return ((g[..., None] - edges.double()).abs() < GHM_MARGIN).any(-1)


def ghm_case(kind, N, C, bins, seed, mu=0.02, shape='spread', labels=False):
    """Inputs of a GHM case.  shape: 'spread' (g over the whole range), 'one_bin' (every valid g inside one bin), 'gaps' (empty bins
    between used ones), 'invalid' (all weights 0).  Weights: GHMC 0 / 1, GHMR 0 / 0.5 / 1 / 2.  ASSERTED: no VALID element's g (the f64
    value) lies within GHM_MARGIN = 1e-5 of an edge; elements that land there by chance are re-drawn until none is left (the device's g
    differs from the f64 one by a few f32 roundings, far inside the margin, so device and statement agree on every bin).
    -> dict(pred, target, weight, edges[, labels, label_weight])."""
    g = _gen(seed)
    edges = ghm_edges(bins, kind)

    def draw(shape_):
        if kind == 'ghmc':
            if shape == 'one_bin':
                return 3.0 + 0.2 * torch.rand(shape_, generator=g)          # target 0: g = sigmoid(x) in (0.95, 0.96)
            if shape == 'gaps':
                return torch.where(torch.rand(shape_, generator=g) < 0.5, -3.0, 3.0) + 0.2 * torch.rand(shape_, generator=g)
            return torch.randn(shape_, generator=g) * 2.5
        if shape == 'one_bin':
            return 5.0 + torch.rand(shape_, generator=g)                     # |d| >> mu: g just below 1
        if shape == 'gaps':
            return torch.where(torch.rand(shape_, generator=g) < 0.5, 0.3, 30.0) * mu * (1 + 0.05 * torch.rand(shape_, generator=g))
        return torch.randn(shape_, generator=g) * 2.0 * mu

    pred = draw((N, C))
    out = dict(edges=edges)
    if kind == 'ghmc':
        if labels:
            lab = torch.randint(0, C + 1, (N,), generator=g)
            lw = (torch.rand(N, generator=g) < 0.8).float()
            target, weight = expand_binary_labels(lab, lw, C)
            out.update(labels=lab, label_weight=lw)
        else:
            target = (torch.rand((N, C), generator=g) < 0.3).float()
            weight = (torch.rand((N, C), generator=g) < 0.8).float()
        if shape in ('one_bin', 'gaps'):
            target = torch.zeros_like(target) if not labels else target
    else:
        target = torch.zeros((N, C))
        weight = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N, C), generator=g)]
        base = torch.randn((N, C), generator=g)
        pred, target = base + pred, base          # d = pred - target is NOT exact here: one f32 rounding, as on the device
    if shape == 'invalid':
        weight = torch.zeros_like(weight)
        if labels:
            out['label_weight'] = torch.zeros_like(out['label_weight'])
    for _ in range(50):
        gv = val(_ghm_g(kind, pred, target, mu, True)[0])
        near = _near_edge(gv, edges) & (weight > 0)
        if not bool(near.any()):
            break
        pred = torch.where(near, pred + (0.013 if kind == 'ghmc' else 0.013 * mu), pred)
    gv = val(_ghm_g(kind, pred, target, mu, True)[0])
    assert not bool((_near_edge(gv, edges) & (weight > 0)).any()), 'a valid element within 1e-5 of a bin edge'
    out.update(pred=pred, target=target, weight=weight)
    return out


def ghmc_edge_case():
    """Hand-made GHMC inputs whose g sits ON edges (outside ghm_case's margin on purpose; for the named mistakes only, never run on a
    device): x = 0 gives g = 0.5 exactly (edge 5 of 10), x = 200 with target 0 gives g = 1 exactly (the last edge but for its + 1e-6)."""
    pred = torch.tensor([[0.0, 200.0, 1.3, -0.7], [0.0, 200.0, -2.1, 0.4]])
    target = torch.tensor([[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0]])
    weight = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 0.0, 1.0]])
    return dict(pred=pred, target=target, weight=weight, edges=ghm_edges(10, 'ghmc'))


# ------------------------------------------------------------------------------------------------ the cases of tests/golden/losses.npz
# (tests/golden/make_losses_golden.py imports them; the tests must not import the maker, whose loader pins the CPU numeric path for the whole process)
PRM = dict(smooth_l1=('beta',), balanced_l1=('beta', 'alpha', 'gamma'), mse=(), iou=('eps',), bounded_iou=('beta', 'eps'))
# every parameter is exact in f32, so the f64 statement (which takes the C floats) and the reference see the same numbers
CASES = dict(smooth_l1=dict(a=((5, 3), dict(beta=1.0)), b=((9, 4), dict(beta=0.125))),
             balanced_l1=dict(a=((5, 3), dict(beta=1.0, alpha=0.5, gamma=1.5)), b=((9, 4), dict(beta=0.5, alpha=0.75, gamma=2.0))),
             mse=dict(a=((5, 3), dict()), b=((9, 4), dict())),
             iou=dict(a=(3, dict(eps=2.0 ** -20)), b=(10, dict(eps=2.0 ** -10))),
             bounded_iou=dict(a=(3, dict(beta=0.25, eps=2.0 ** -10)), b=(10, dict(beta=0.125, eps=2.0 ** -7))))
GHM_RUNS = dict(ghmc_m0=('ghmc', 10, 0.0, 1.0, True), ghmc_m75=('ghmc', 10, 0.75, 2.0, False),
                ghmr_m0=('ghmr', 10, 0.0, 1.0, False), ghmr_m75=('ghmr', 10, 0.75, 0.5, False))
GHM_SHAPE, GHM_MU, AVG = (12, 4), 2.0 ** -6, 7.0
