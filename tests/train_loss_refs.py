"""Plain float64 statements of the ARITHMETIC kernels of the training step, written independently of the HIP code, with the error
bounds that tests/test_train_loss_refs.py (CPU) and tests/test_train_losses_gpu.py (GPU) hold the kernels to:

  det_loss_kernel (plain and OHEM form), rpn_loss_kernel, ce_rows_kernel, hvr_relation_probs (score pass + normalising sweep),
  relation_dscore_kernel, sumsq / sgd_step kernels, relu_bwd_kernel, scale_rows_kernel.

Every function takes the kernel's own f32 (bf16 / half) inputs on any device and returns (reference, bound) in float64, the bound
per output element.  Scalars the kernels receive as `float` (beta, lr, scale, 1e-6f ...) enter the statement with their f32 value
(f32v), so that the reference is the exact function of what the kernel was given.

Error model.  u = 2^-24 is the unit roundoff of f32; one f32 operation (+ - * and a fused multiply-add) has relative error <= u.
A sum of n terms added in ANY order whose longest chain of additions is c has error <= c u sum|term| to first order.  The bounds
are first-order sums of such terms, multiplied by SECOND = 1 + 2^-10 for the products of errors they drop (every coefficient of u
used here is far below 2^10), plus TINY = 2^-126 per element for results that f32 flushes or rounds in its subnormal range (an
exponential that underflows).  A bound never contains a value measured on the device.

Device math functions.  No accuracy table of the device math library ships with the ROCm documentation installed next to the
compiler (share/doc holds the runtime API reference only), so the constants below are the limits the OpenCL full profile sets
for the same built-ins, which the device library (OCML) implements and HIP's expf / logf / log1pf / exp2f / sqrtf lower to:
exp, exp2, log <= 3 ulp, log1p <= 2 ulp, sqrt <= 3 ulp, x / y <= 2.5 ulp.  One ulp is at most 2 u relative.  The score pass calls
the hardware exponential (v_exp_f32) directly: 1 ulp in the CDNA ISA guide, subnormal results flushed (TINY).  Their exact size
matters little: the CPU tests show every bound wide enough for an independent f32 evaluation and every listed mistake at least
ten times larger than it.
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -10
EXPF_ULP = 3.0
EXP2F_ULP = 3.0
LOGF_ULP = 3.0
LOG1PF_ULP = 2.0
SQRTF_ULP = 3.0
DIV_ULP = 2.5
V_EXP_ULP = 1.0
ULP = 2.0 * U            # relative size of one ulp, at most


def f32v(x):
    """The value a C `float` argument takes."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _lse_parts(x):
    """x [R, ncls] f64 -> (lse, E_lse): log-sum-exp and the bound on the kernels' `mx + logf(se)`.
    se = sum_c expf(x_c - mx), added in sequence: x_c - mx has error u t_c (t_c = mx - x_c) which the exponential turns into a
    relative error t_c u of the term, expf adds EXPF_ULP ulp, the ncls - 1 additions (ncls - 1) u: relative error of se
      d_se = (ncls - 1 + 2 EXPF_ULP) u + u sum_c t_c e^-t_c / se.
    logf(se) then has absolute error d_se + 2 LOGF_ULP u |log se|, and the sum mx + logf(se) is rounded once: u |lse|."""
    mx = x.max(1).values
    t = mx[:, None] - x
    e = torch.exp(-t)
    se = e.sum(1)
    d_se = (x.shape[1] - 1 + 2 * EXPF_ULP) * U + U * (t * e).sum(1) / se
    lse = mx + torch.log(se)
    return lse, d_se + 2 * LOGF_ULP * U * torch.log(se).abs() + U * lse.abs()


def ce_rows_statement(logits, cls_off, ncls, labels):
    """ce_rows_kernel: loss[r] = logsumexp(x_r) - x_r[label_r].  Bound: E_lse + u |loss| (the final subtraction) + TINY."""
    x = logits[:, cls_off:cls_off + ncls].double()
    assert int(labels.min()) >= 0 and int(labels.max()) < ncls, 'labels outside [0, ncls): the kernels do not check'
    lse, e_lse = _lse_parts(x)
    ce = lse - x.gather(1, labels.view(-1, 1)).squeeze(1)
    return ce, SECOND * (e_lse + U * ce.abs()) + TINY


def block_chain(n, lanes, levels):
    """Longest chain of additions behind a one-workgroup sum: lane t adds terms t, t + lanes, ... (the first onto 0 is exact),
    then a `levels`-level tree."""
    return -(-n // lanes) + levels


def _smooth_l1(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta), torch.where(a < beta, d / beta, torch.sign(d))


def _top1_untied(x):
    """argmax per row, asserting that no row's two largest logits tie (the accuracy is compared as an exact count)."""
    if x.shape[1] > 1:
        top = x.topk(2, dim=1).values
        assert bool((top[:, 0] > top[:, 1]).all()), 'two largest class logits of a row tie: change the case'
    return x.argmax(1)


def det_loss_statement(logits, cls_off, reg_off, ncls, labels, label_w, bbox_t, bbox_w, beta=1.0, w_cls=1.0, w_bbox=1.0,
                       sel_counts=None, mistake=None):
    """det_loss_kernel (BBoxHead.loss, class-agnostic boxes) -> dict(out3 [3], dlogits [R, ldl], count) and the same dict of bounds.
      loss_cls = sum_r ce_r w_r / avg,            avg = max(#{w > 0}, 1)
      loss_bbox = sum_{r: label_r > 0} sum_e smoothL1_beta(pred_re - target_re) bw_re / rows,
                  rows = R, or max(sel_counts[0] + sel_counts[1], 1) in the sampled (OHEM) form
      acc = 100 #{r: argmax x_r = label_r [and w_r > 0 in the sampled form]} / rows       (`count` = that number, exact)
      dlogits = d(w_cls loss_cls + w_bbox loss_bbox) / d logits, zero outside the class and delta columns.
    Bounds (E_lse, d_se from _lse_parts; chain = ceil(R / 256) + 8: thread t adds rows t, t + 256, ..., then an 8-level tree):
      ce_r w_r: |w| (E_lse + 2 u |ce|);  loss_cls: [(chain + 1 + 2 DIV_ULP) u sum|ce w| + sum|w| (E_lse + 2 u |ce|)] / avg.
      smooth-L1 term: d = pred - target is rounded (u |d|, and the loss is 1-Lipschitz in d), 0.5 a a / beta * bw is three
      roundings and a division, a - 0.5 beta two: |bw| u (|d| + (3 + 2 DIV_ULP) l1); summed and divided like loss_cls.
      A multiply-add contracted into one fma only drops a rounding, so the bounds hold with and without contraction.
      acc: count (an integer below 2^24: exact) times 100 / rows: (1 + 2 DIV_ULP) u |acc|.
      class gradient  w_cls w / avg (expf(x_c - lse) - [c = label]):  p = expf(x_c - lse) has relative error
        E_lse + u |x_c - lse| + 2 EXPF_ULP u, kept as p * (...) because p - 1 cancels; the subtraction adds u |p - 1|; the
        coefficient is two roundings and a division: (2 + 2 DIV_ULP) u |g|.
      box gradient  w_bbox bw / rows (d / beta or sign d): coefficient as above, d: u, d / beta: 2 DIV_ULP u; a d whose rounding
        moves it across beta changes the factor by at most 2 u (the two forms meet at |d| = beta): coef 2 u.
    mistake: one of the plausible kernel mistakes named in MISTAKES_DET, applied to the statement (CPU tests only)."""
    R = logits.shape[0]
    beta = f32v(beta)
    x = logits[:, cls_off:cls_off + ncls].double()
    assert int(labels.min()) >= 0 and int(labels.max()) < ncls, 'labels outside [0, ncls): the kernels do not check'
    w, bw = label_w.double(), bbox_w.double().view(R, 4)
    lse, e_lse = _lse_parts(x)
    if mistake == 'lse_without_max':                      # f32 exp overflows where the kernel's shifted form cannot
        lse = torch.log(torch.exp(logits[:, cls_off:cls_off + ncls].float()).sum(1)).double()
    ce = lse - x.gather(1, labels.view(-1, 1)).squeeze(1)
    avg = max(float((label_w > 0).sum()), 1.0)
    if mistake == 'avg_is_R':
        avg = float(R)
    sampled = sel_counts is not None
    rows = float(max(int(sel_counts[0]) + int(sel_counts[1]), 1)) if sampled else float(R)
    if mistake == 'sampled_bbox_over_R':
        rows = float(R)
    chain = block_chain(R, 256, 8)
    tc = ce * w
    loss_cls = tc.sum() / avg
    e_tc = w.abs() * (e_lse + 2 * U * ce.abs())
    b_cls = ((chain + 1 + 2 * DIV_ULP) * U * tc.abs().sum() + e_tc.sum()) / avg

    pos = (labels > 0).double()[:, None]
    if mistake == 'no_label_gate':
        pos = torch.ones_like(pos)
    d = logits[:, reg_off:reg_off + 4].double() - bbox_t.double().view(R, 4)
    l1, dl1 = _smooth_l1(d, beta)
    if mistake == 'no_div_beta':
        l1 = torch.where(d.abs() < beta, 0.5 * d * d, d.abs() - 0.5 * beta)
    tb = l1 * bw * pos
    loss_bbox = tb.sum() / rows
    e_tb = bw.abs() * pos * U * (d.abs() + (3 + 2 * DIV_ULP) * l1)
    b_bbox = ((chain + 1 + 2 * DIV_ULP) * U * tb.abs().sum() + e_tb.sum()) / rows

    hit = _top1_untied(x) == labels
    if sampled and mistake != 'sampled_acc_all_rows':
        hit = hit & (label_w > 0)
    count = int(hit.sum())
    acc = count * 100.0 / rows

    dl = torch.zeros(logits.shape, dtype=torch.float64, device=logits.device)
    bd = torch.zeros_like(dl)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, labels.view(-1, 1), 1.0)
    coef = (f32v(w_cls) * w / avg)[:, None]
    g = coef * (p - onehot)
    rel_p = (e_lse[:, None] + U * (x - lse[:, None]).abs() + 2 * EXPF_ULP * U)
    dl[:, cls_off:cls_off + ncls] = g
    bd[:, cls_off:cls_off + ncls] = SECOND * (coef.abs() * (p * rel_p + U * (p - onehot).abs() + TINY) + (2 + 2 * DIV_ULP) * U * g.abs())
    cb = f32v(w_bbox) * bw / rows * pos
    gb = cb * dl1
    dl[:, reg_off:reg_off + 4] = gb
    bd[:, reg_off:reg_off + 4] = SECOND * ((3 + 4 * DIV_ULP) * U * gb.abs() + 2 * U * cb.abs())
    ref = dict(out3=torch.stack([loss_cls, loss_bbox, torch.tensor(acc, dtype=torch.float64, device=logits.device)]), dlogits=dl, count=count,
               rows=rows)
    bound = dict(out3=torch.stack([SECOND * b_cls + TINY, SECOND * b_bbox + TINY,
                                   torch.tensor((1 + 2 * DIV_ULP) * U * acc * SECOND, dtype=torch.float64, device=logits.device)]),
                 dlogits=bd)
    return ref, bound


MISTAKES_DET = ('avg_is_R', 'no_div_beta', 'no_label_gate', 'lse_without_max')
MISTAKES_DET_SAMPLED = ('sampled_bbox_over_R', 'sampled_acc_all_rows')


def det_loss_f32(logits, cls_off, reg_off, ncls, labels, label_w, bbox_t, bbox_w, beta=1.0, w_cls=1.0, w_bbox=1.0, sel_counts=None):
    """The same statement evaluated by plain PyTorch in f32 (autograd for the gradient): an independent order of operations."""
    import torch.nn.functional as F
    R = logits.shape[0]
    lg = logits.clone().float().requires_grad_(True)
    avg = max(float((label_w > 0).sum()), 1.0)
    rows = float(max(int(sel_counts[0]) + int(sel_counts[1]), 1)) if sel_counts is not None else float(R)
    loss_cls = (F.cross_entropy(lg[:, cls_off:cls_off + ncls], labels, reduction='none') * label_w.float()).sum() / avg
    pos = labels > 0
    diff = lg[:, reg_off:reg_off + 4][pos] - bbox_t.float().view(R, 4)[pos]
    b = torch.tensor(beta, dtype=torch.float32)
    l1 = torch.where(diff.abs() < b, 0.5 * diff * diff / b, diff.abs() - 0.5 * b)
    loss_bbox = (l1 * bbox_w.float().view(R, 4)[pos]).sum() / rows
    (torch.tensor(w_cls, dtype=torch.float32) * loss_cls + torch.tensor(w_bbox, dtype=torch.float32) * loss_bbox).backward()
    hit = lg[:, cls_off:cls_off + ncls].argmax(1) == labels
    if sel_counts is not None:
        hit = hit & (label_w > 0)
    acc = hit.float().sum() * (100.0 / rows)
    return dict(out3=torch.stack([loss_cls.detach(), loss_bbox.detach(), acc]), dlogits=lg.grad)


def det_case(R, layout, beta, seed, kind='plain', logit_scale=3.0):
    """One input set of the det-loss tests (CPU tensors).  layout = (ldl, cls_off, reg_off, ncls).  Rows: about a quarter of
    the labels positive, background rows WITH non-zero box weights (the label > 0 gate), label weights 0 on about a third of
    the rows, deltas on every branch point of smooth-L1 -- target +- beta, +- beta (1 +- 2^-20), equal to the target (targets
    of those rows are multiples of 1/4 or zero so that pred - target is exactly that) -- and, when R allows, one row of logits
    at +-1e4.  kind: 'plain', 'no_pos' (no label > 0), 'zero_w' (all label weights zero), 'big' (logits scaled to +-80)."""
    ldl, cls_off, reg_off, ncls = layout
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((R, ldl), generator=g) * logit_scale
    if kind == 'big':
        x = logits[:, cls_off:cls_off + ncls]
        logits[:, cls_off:cls_off + ncls] = x / x.abs().max() * 80.0
    labels = torch.randint(1, ncls, (R,), generator=g) * (torch.rand(R, generator=g) < 0.25).long()
    if R >= 4:
        labels[1] = 1                                     # at least one positive and one background row
        labels[2] = 0
    if kind == 'no_pos':
        labels.zero_()
    label_w = (torch.rand(R, generator=g) < 0.67).float() * (0.5 + torch.rand(R, generator=g))
    if kind == 'zero_w':
        label_w.zero_()
    bbox_t = torch.randn((R, 4), generator=g)
    bbox_w = 0.5 + torch.rand((R, 4), generator=g)       # background rows too: only the label gate keeps them out
    b32 = torch.tensor(beta, dtype=torch.float32)
    # branch points, on positive rows
    pts = [b32, -b32, b32 * (1 + 2.0 ** -20), b32 * (1 - 2.0 ** -20), -b32 * (1 + 2.0 ** -20), -b32 * (1 - 2.0 ** -20), torch.tensor(0.0)]
    rows = torch.nonzero(labels > 0).flatten()[: len(pts)]
    for i, r in enumerate(rows.tolist()):
        bbox_t[r] = 0.0
        logits[r, reg_off:reg_off + 4] = pts[i]
    if R >= 64 and kind != 'big':
        r = int(torch.nonzero(labels > 0).flatten()[-1]) if kind != 'no_pos' else R - 1
        logits[r, cls_off:cls_off + ncls] = torch.where(torch.arange(ncls) % 2 == 0, 1e4, -1e4) + torch.arange(ncls).float()
        if kind != 'no_pos':
            labels[r] = ncls - 1 if (ncls - 1) % 2 else ncls - 2      # an odd column: its logit is -1e4, the loss about 2e4
        if kind != 'zero_w':
            label_w[r] = 1.0
    _top1_untied(logits[:, cls_off:cls_off + ncls].double())
    return dict(logits=logits, cls_off=cls_off, reg_off=reg_off, ncls=ncls, labels=labels, label_w=label_w, bbox_t=bbox_t,
                bbox_w=bbox_w, beta=beta)


DET_LAYOUTS = [(36, 0, 31, 31), (40, 4, 0, 31), (64, 8, 48, 2)]
DET_ROWS = [1, 255, 256, 257, 4500, 20000]


def det_params():
    """Every input set of the det-loss tests as (id, dict(R, layout, beta, kind, sel)); sel None = plain form, else the sampled
    form with sel_counts 'real' / 'zero' / 'neg_only'."""
    out = []
    for li, layout in enumerate(DET_LAYOUTS):
        for R in DET_ROWS:
            for beta in (1.0, 1.0 / 9.0):
                out.append(dict(R=R, layout=layout, beta=beta, kind='plain', sel=None))
            out.append(dict(R=R, layout=layout, beta=1.0 if li % 2 else 1.0 / 9.0, kind='plain', sel='real'))
    for R in (257, 4500):
        for kind in ('no_pos', 'zero_w', 'big'):
            out.append(dict(R=R, layout=DET_LAYOUTS[0], beta=1.0 / 9.0, kind=kind, sel=None))
            out.append(dict(R=R, layout=DET_LAYOUTS[1], beta=1.0, kind=kind, sel='real'))
        for sel in ('zero', 'neg_only'):
            out.append(dict(R=R, layout=DET_LAYOUTS[0], beta=1.0, kind='plain', sel=sel))
    return [('R%d-l%d-b%s-%s-%s' % (p['R'], DET_LAYOUTS.index(p['layout']), 'one' if p['beta'] == 1.0 else 'ninth', p['kind'], p['sel'] or 'plain'), p)
            for p in out]


def det_build(p):
    """(case dict for det_loss_statement / native.det_loss[_sampled], sel_counts tuple or None) of one det_params() entry.  In the
    sampled form the rows outside the selection carry zero weights (the entry point's contract): box weights follow the label
    weights there; selected background rows keep theirs."""
    seed = p['R'] * 7 + DET_LAYOUTS.index(p['layout']) + (3 if p['beta'] == 1.0 else 0) + len(p['kind'])
    case = det_case(p['R'], p['layout'], p['beta'], seed, p['kind'])
    if p['sel'] is None:
        return case, None
    case['bbox_w'] = case['bbox_w'] * (case['label_w'] > 0).float()[:, None]
    return case, sel_counts_for(case, p['sel'])


def sel_counts_for(case, which):
    """sel_counts of the sampled form for a det case: 'real' = (#selected positives, #selected negatives) of its weights;
    'zero' = (0, 0); 'neg_only' = (0, n)."""
    sel = case['label_w'] > 0
    if which == 'zero':
        return (0, 0)
    if which == 'neg_only':
        return (0, int(sel.sum()))
    return (int((sel & (case['labels'] > 0)).sum()), int((sel & (case['labels'] == 0)).sum()))


# ------------------------------------------------------------------------------------------------ rpn loss
def rpn_loss_statement(o, A, labels, label_w, bbox_t, bbox_w, counts, beta, mistake=None):
    """rpn_loss_kernel on the fused head output o [rows, ldo] (A logits, then 4 deltas per anchor from column A) -> dict(out2,
    d_o) and bounds.  M = rows * A terms, m = r A + a:
      loss_cls = sum_m bce(x_m, z_m) w_m / avg,   bce = max(x, 0) - x z + log1p(exp(-|x|)),   avg = max(c0, 1) + max(c1, 1)
      loss_bbox = sum_m sum_e smoothL1_beta(pred - target) bw / avg;      d_o = d(loss_cls + loss_bbox) / d o, zero elsewhere.
    Bounds (chain = ceil(M / 1024) + 10; contraction is off in this file, the bounds do not rely on it):
      bce term: ex = expf(-|x|) (2 EXPF_ULP u ex, flushed below TINY), log1pf(ex): slope <= 1 in ex, 2 LOG1PF_ULP u log1p(ex);
        max(x, 0) - x z is exact for z in {0, 1}; the sum and the product with w: 2 u |bce|.
      sigmoid (1 or ex) / (1 + ex): (2 EXPF_ULP + 1 + 2 DIV_ULP) u sig, then (sig - z) w / avg: u |sig - z| and (1 + 2 DIV_ULP) u |g|.
      smooth-L1 and its gradient as in det_loss_statement."""
    rows, ldo = o.shape
    beta = f32v(beta)
    M = rows * A
    x = o[:, :A].double().reshape(-1)
    z, w = labels.double().reshape(-1), label_w.double().reshape(-1)
    c0, c1 = int(counts[0]), int(counts[1])
    avg = float(max(c0, 1) + max(c1, 1))
    if mistake == 'avg_without_max':
        avg = float(c0 + c1)
    ex = torch.exp(-x.abs())
    bce = x.clamp(min=0) - x * z + torch.log1p(ex)
    chain = block_chain(M, 1024, 10)
    tcl = bce * w
    e_t = w.abs() * (2 * EXPF_ULP * U * ex + 2 * LOG1PF_ULP * U * torch.log1p(ex) + 2 * U * bce.abs() + TINY)
    loss_cls = tcl.sum() / avg
    b_cls = ((chain + 1 + 2 * DIV_ULP) * U * tcl.abs().sum() + e_t.sum()) / avg
    d = o[:, A:5 * A].double().reshape(M, 4) - bbox_t.double().reshape(M, 4)
    bw = bbox_w.double().reshape(M, 4)
    l1, dl1 = _smooth_l1(d, beta)
    if mistake == 'no_div_beta':
        l1 = torch.where(d.abs() < beta, 0.5 * d * d, d.abs() - 0.5 * beta)
    tb = l1 * bw
    loss_bbox = tb.sum() / avg
    e_tb = bw.abs() * U * (d.abs() + (3 + 2 * DIV_ULP) * l1)
    b_bbox = ((chain + 1 + 2 * DIV_ULP) * U * tb.abs().sum() + e_tb.sum()) / avg
    sig = torch.where(x >= 0, 1 / (1 + ex), ex / (1 + ex))
    if mistake == 'sigmoid_one_branch':                   # the x >= 0 formula 1 / (1 + ex), ex = exp(-|x|), used on both sides
        sig = 1 / (1 + ex)
    dx = torch.zeros(o.shape, dtype=torch.float64, device=o.device)
    bd = torch.zeros_like(dx)
    gc = (sig - z) * w / avg
    dx[:, :A] = gc.view(rows, A)
    bd[:, :A] = (SECOND * ((w / avg).abs() * ((2 * EXPF_ULP + 1 + 2 * DIV_ULP) * U * sig + U * (sig - z).abs() + TINY)
                           + (1 + 2 * DIV_ULP) * U * gc.abs())).view(rows, A)
    cb = bw / avg
    gb = cb * dl1
    dx[:, A:5 * A] = gb.view(rows, 4 * A)
    bd[:, A:5 * A] = (SECOND * ((2 + 4 * DIV_ULP) * U * gb.abs() + 2 * U * cb.abs())).view(rows, 4 * A)
    return (dict(out2=torch.stack([loss_cls, loss_bbox]), d_o=dx),
            dict(out2=torch.stack([SECOND * b_cls + TINY, SECOND * b_bbox + TINY]), d_o=bd))


MISTAKES_RPN = ('avg_without_max', 'no_div_beta', 'sigmoid_one_branch')


def rpn_loss_f32(o, A, labels, label_w, bbox_t, bbox_w, counts, beta):
    import torch.nn.functional as F
    rows = o.shape[0]
    M = rows * A
    of = o.clone().float().requires_grad_(True)
    avg = float(max(int(counts[0]), 1) + max(int(counts[1]), 1))
    lc = (F.binary_cross_entropy_with_logits(of[:, :A].reshape(-1), labels.float().reshape(-1), reduction='none') * label_w.float().reshape(-1)).sum() / avg
    diff = (of[:, A:5 * A].reshape(M, 4) - bbox_t.float().reshape(M, 4)).abs()
    b = torch.tensor(beta, dtype=torch.float32)
    lb = (torch.where(diff < b, 0.5 * diff * diff / b, diff - 0.5 * b) * bbox_w.float().reshape(M, 4)).sum() / avg
    (lc + lb).backward()
    return dict(out2=torch.stack([lc.detach(), lb.detach()]), d_o=of.grad)


RPN_SHAPES = [(2394, 12, 64), (4200, 12, 64), (1, 1, 5), (7, 3, 15), (2394, 9, 48)]
RPN_COUNTS = [(0, 0), (0, 256), (128, 128)]


def rpn_case(rows, A, ldo, counts, seed, beta=1.0 / 9.0, big=False):
    """Input set of the rpn-loss tests: c0 positives (label 1, box weights 1) and c1 negatives carry label weight 1 (as many as
    fit), every anchor a box weight on a tenth of the rest too (the kernel has no gate: weights decide), objectness logits
    N(0, 3) or, with big, scaled to +-90 (both sigmoid branches at large magnitude, x = 0 on purpose), deltas on the smooth-L1
    branch points."""
    g = torch.Generator().manual_seed(seed)
    M = rows * A
    o = torch.randn((rows, ldo), generator=g) * 3.0
    if big:
        o[:, :A] = o[:, :A] / o[:, :A].abs().max() * 90.0
    labels = torch.zeros(M, dtype=torch.long)
    label_w = torch.zeros(M)
    bbox_w = torch.zeros((M, 4))
    perm = torch.randperm(M, generator=g)
    c0, c1 = min(counts[0], M // 2), min(counts[1], M - M // 2)
    labels[perm[:c0]] = 1
    label_w[perm[:c0 + c1]] = 1.0
    bbox_w[perm[:c0]] = 1.0
    extra = perm[c0 + c1:][: max(1, M // 10)] if M > c0 + c1 else perm[:1]
    bbox_w[extra] = 0.5
    label_w[extra[:1]] = 0.25
    bbox_t = torch.randn((M, 4), generator=g)
    b32 = torch.tensor(beta, dtype=torch.float32)
    pts = [b32 * (1 - 2.0 ** -20), -b32 * (1 - 2.0 ** -20), b32, -b32, b32 * (1 + 2.0 ** -20), -b32 * (1 + 2.0 ** -20), torch.tensor(0.0)]
    picks = torch.nonzero(bbox_w[:, 0] > 0).flatten()[: len(pts)]
    ov = o[:, A:5 * A].reshape(M, 4).clone()
    for i, m in enumerate(picks.tolist()):
        bbox_t[m] = 0.0
        ov[m] = pts[i]
    o[:, A:5 * A] = ov.view(rows, 4 * A)
    if M >= 2:
        o.view(-1)[(perm[0] // A) * ldo + perm[0] % A] = 0.0        # BCE exactly at x = 0
    return dict(o=o, A=A, labels=labels, label_w=label_w, bbox_t=bbox_t, bbox_w=bbox_w, counts=torch.tensor(counts, dtype=torch.int32),
                beta=beta)


# ------------------------------------------------------------------------------------------------ relation probabilities
UNIT = {torch.float32: U, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # unit roundoff of the storage type (8 / 11 significant bits)
SUBNORMAL_HALF_STEP = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}   # half a step of half's subnormal grid


def relation_probs_statement(q, k, scale, mistake=None):
    """hvr_relation_probs: P = softmax(scale q k^T) [Mq, ldp] with exact zeros in columns Mk .. ldp (ldp = Mk rounded up to 128).
    -> (P f64, bound f64, blocks) where `bound` is on the f32 value the kernel holds before the final store.
    The kernel: raw dot products a_j (f32 accumulation over D: |error| <= g_D |q|.|k_j|, g_D = D u / (1 - D u)); per 128-key
    block t the maximum m_t; P~_j = exp2(a_j sl2 - m_t) with sl2 = fl(scale log2 e); l_t = sum of the block's P~; then
    P_j = P~_j * [exp2f(m_t - m*) / sum_t l_t exp2f(m_t - m*)].  In units of the natural logarithm:
      * the dot-product error moves every exponent of the row by at most E_s = max_j scale g_D |q|.|k_j|.  With d_k in [-E_s, E_s],
        P'_j = P_j e^d_j / sum_k P_k e^d_k lies between P_j / (P_j + (1 - P_j) e^(+-2 E_s)), so
        |P'_j - P_j| <= P_j (1 - P_j) (e^(2 E_s) - 1) exactly: relative 2 E_s for small P_j, and next to nothing for a P_j close
        to one (its own error cancels against the denominator's);
      * sl2 is off by <= 2 u relative, the fused multiply-add and m_t - m* are rounded: <= 4 u (m* - s_j) on P_j's exponent
        (`gap_j`), and 4 u sum_k P_k gap_k on the denominator's (the rounding of m_t itself cancels: both passes use the stored
        value);
      * roundings: numerator 2 V_EXP_ULP + 2 EXP2F_ULP + 2 DIV_ULP + 1 = 14 u; a block sum l_t is <= 16 additions of terms with
        2 V_EXP_ULP u each, times exp2f: 25 u; the sum over blocks: lane chain ceil(nt / 64) and 6 butterfly levels.
      bound = SECOND P ((1 - P) expm1(2 E_s) + 4 u gap + 4 u G + (45 + ceil(nt / 64)) u) + TINY.
    A two-byte P is rounded twice -- P~ to the type, then the product with the block factor -- see relation_probs_bracket.
    mistake 'neighbour_max': block t normalised with block t + 1's maximum (the last with the first's)."""
    Mq, D = q.shape
    Mk = k.shape[0]
    ldp = (Mk + 127) // 128 * 128
    nt = ldp // 128
    sc = f32v(scale)
    S = torch.full((Mq, ldp), -float('inf'), dtype=torch.float64, device=q.device)
    S[:, :Mk] = sc * (q.double() @ k.double().t())
    absdot = q.double().abs() @ k.double().abs().t()
    gD = D * U / (1 - D * U)
    Es = (sc * gD * absdot).max(1).values[:, None]
    mstar = S.max(1).values[:, None]
    gap = torch.where(torch.isinf(S), torch.zeros_like(S), mstar - S)
    e = torch.exp(S - mstar)
    if mistake == 'neighbour_max':
        mt = S.view(Mq, nt, 128).max(2).values                      # [Mq, nt]
        shift = (mt - mt.roll(-1, 1)).clamp(min=-700, max=700)      # a block of padding only cannot be a neighbour here: nt from Mk
        e = (e.view(Mq, nt, 128) * torch.exp(shift)[:, :, None]).view(Mq, ldp)
    L = e.sum(1, keepdim=True)
    P = e / L
    G = (P * gap).sum(1, keepdim=True)
    # 1 - P without cancellation: for the row's largest element the sum of the others, elsewhere (P <= 1/2) the plain difference
    top = e.argmax(1, keepdim=True)
    others = e.scatter(1, top, 0.0).sum(1, keepdim=True) / L
    om = (1 - P).scatter(1, top, others)
    bound = SECOND * P * (om * torch.expm1(2 * Es) + 4 * U * gap + 4 * U * G + (45 + -(-nt // 64)) * U) + TINY
    bound[:, Mk:] = 0.0                                              # padding: exactly zero
    return P, bound, nt


def relation_probs_bracket(P, bound, dtype):
    """[lo, hi] (f32 tensors of values of `dtype`) that the stored P must lie in.  f32: P -+ bound.  bf16 / half: the score pass
    stores P~ rounded to the type (relative u_T, and for half an absolute 2^-25 in its subnormal range, scaled by a block factor
    <= 1), the sweep multiplies by the block factor in f32 and rounds again.  The f32 product therefore lies within
    b' = bound + u_T P (1 + bound / P) + 2^-25 of P, and rounding is monotone: the stored value lies between the roundings of
    P - b' and P + b'."""
    if dtype == torch.float32:
        return (P - bound), (P + bound)
    b2 = bound + UNIT[dtype] * (P + bound) + torch.where(bound > 0, torch.full_like(P, SUBNORMAL_HALF_STEP[dtype]), torch.zeros_like(P))
    lo, hi = _round_down_f32(P - b2), _round_up_f32(P + b2)
    return lo.to(dtype).double(), hi.to(dtype).double()


def _round_down_f32(x):
    """largest f32 <= x (x f64), so that a following f32 -> dtype rounding brackets from the outside"""
    f = x.float()
    return torch.where(f.double() > x, torch.nextafter(f, torch.full_like(f, -float('inf'))), f)


def _round_up_f32(x):
    f = x.float()
    return torch.where(f.double() < x, torch.nextafter(f, torch.full_like(f, float('inf'))), f)


def bracket(ref, bound, dtype):
    """Single rounding of an f32 value within `bound` of `ref` to dtype (monotone): [round(ref - bound), round(ref + bound)]."""
    if dtype == torch.float32:
        return ref - bound, ref + bound
    return _round_down_f32(ref - bound).to(dtype).double(), _round_up_f32(ref + bound).to(dtype).double()


def relation_inputs(Mq, Mk, D, dtype, seed, device='cpu', pad=0, peaky=True):
    """q [Mq, D], k [Mk, D] N(0, 1) in dtype, as row slices of matrices `pad` columns wider (ldq, ldk > D when pad > 0).  With
    peaky (and Mk >= 2): row 0 of q and key Mk - 1 are 4 x one sign pattern, so that row's maximum stands scale 16 D above the
    other blocks' (at D = 1024 and scale 1/32: 512, beyond the exponent range of f32's exp2), and row Mq // 2 / key 0 share a
    unit pattern (a gap of scale D: blocks whose factors are tiny but not zero)."""
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn((Mq, D + pad), generator=g)
    K = torch.randn((Mk, D + pad), generator=g)
    if peaky and Mk >= 2:
        s = torch.sign(torch.randn(D, generator=g))
        Q[0, :D], K[Mk - 1, :D] = 4 * s, 4 * s
        s2 = torch.sign(torch.randn(D, generator=g))
        if Mq > 1:
            Q[Mq // 2, :D], K[0, :D] = s2, s2
    Q, K = Q.to(dtype).to(device), K.to(dtype).to(device)
    return Q[:, :D], K[:, :D]


RELATION_MK = [1, 37, 127, 128, 129, 4100, 4500, 8192, 8320]
RELATION_MQ = [1, 37, 300]
RELATION_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MAX_KEYS = 16384                                            # 128 blocks of 128 keys: the normalising sweep's table


def relation_dscore_statement(P, dP, dO, O, scale, mistake=None):
    """relation_dscore_kernel: dS = scale P (dP - delta), delta_m = sum_d dO[m, d] O[m, d].
    delta: thread t adds, per step of 1 024 columns, (p0 + p1) + (p2 + p3) onto its partial (chain 3 ceil(D / 1024), products
    rounded or fused: + 1), a 64-lane butterfly (6), four partials (2): E_delta = (3 ceil(D / 1024) + 9) u sum|dO O|.
    dP - delta: u |dP - delta| on top of E_delta -- the cancellation is why the bound carries sum|dO O| and not |dS| --
    then two products: bound = SECOND [|scale P| (E_delta + u |dP - delta|) + 2 u |dS|] + TINY, on the f32 value before the store."""
    sc = f32v(scale)
    D = dO.shape[1]
    prod = dO.double() * O.double()
    delta = prod.sum(1, keepdim=True)
    if mistake == 'no_delta':
        delta = torch.zeros_like(delta)
    e_delta = (3 * -(-D // 1024) + 9) * U * prod.abs().sum(1, keepdim=True)
    diff = dP.double() - delta
    dS = sc * P.double() * diff
    bound = SECOND * ((sc * P.double()).abs() * (e_delta + U * diff.abs()) + 2 * U * dS.abs()) + TINY
    return dS, bound


# ------------------------------------------------------------------------------------------------ sgd step
SUMSQ_PARTS = 1024
GRID_CAP_THREADS = 4096 * 256        # misc.hip grid_for: at most 4 096 workgroups of 256; more work items than that loop (grid stride)


def sumsq_chain(n):
    """Longest chain of additions behind the sum of squares: a lane adds 4 squares per float4 step (ceil(n4 / (1024 * 256))
    steps) and possibly one tail element, an 8-level tree, then 1 024 partials over 256 lanes (4) and another 8-level tree."""
    n4 = n // 4
    return 4 * -(-n4 // (SUMSQ_PARTS * 256)) + 1 + 8 + 4 + 8


def sgd_statement(p, g, buf, lr, mom, wd, gscale=1.0, max_norm=0.0, first=False, mistake=None):
    """hvr_sgd_step, ONE call -> ((p', buf'), (bound_p, bound_buf), clip).
      clip = min(1, max_norm / (|g| gscale + 1e-6)) if max_norm > 0 else 1          (the norm of the AVERAGED gradient)
      d = g gscale clip + wd p;   buf' = d if first else mom buf + d;   p' = p - lr buf'
    The sum of squares has only positive terms: relative error (sumsq_chain + 1) u =: d_ss.  norm = sqrtf(ss) gscale:
    d_ss / 2 + (2 SQRTF_ULP + 1) u; + 1e-6: u; the division: 2 DIV_ULP u  ->  d_c.  min(., 1) is continuous, so d_c applies
    wherever the reference coefficient is below 1 + 2 d_c and nothing beyond.  k = gscale clip: u.  Then
      E_d = |g k| (d_c + 2 u) + 2 u |wd p| + u |d|;  E_buf = E_d + u |mom buf| + u |buf'|  (first: E_d);
      E_p = |lr| E_buf + u |lr buf'| + u |p'|.
    A contracted multiply-add drops a rounding; the bounds hold either way."""
    lr, mom, wd, gs, mn = f32v(lr), f32v(mom), f32v(wd), f32v(gscale), f32v(max_norm)
    P, Gd, B = p.double(), g.double(), buf.double()
    n = p.numel()
    clip, d_c = 1.0, 0.0
    if mn > 0:
        gg = Gd
        if mistake == 'tail_dropped':
            gg = Gd[: n // 4 * 4]
        norm = math.sqrt(float((gg * gg).sum())) * (1.0 if mistake == 'norm_unaveraged' else gs)
        c = mn / (norm + f32v(1e-6))
        d_ss = (sumsq_chain(n) + 1) * U
        d_c = d_ss / 2 + (2 * SQRTF_ULP + 2 + 2 * DIV_ULP) * U
        if c >= 1 + 2 * d_c:
            d_c = 0.0
        clip = min(c, 1.0)
    kk = gs * clip
    if mistake == 'wd_after_momentum':
        d = Gd * kk
        b = d if first else mom * B + d
        b_out = b
        p_new = P - lr * (b + wd * P)
    else:
        d = Gd * kk + wd * P
        b = mom * B + d if (not first or mistake == 'stale_first') else d
        b_out = b
        p_new = P - lr * b
    e_d = (Gd * kk).abs() * (d_c + 2 * U) + 2 * U * (wd * P).abs() + U * d.abs()
    e_b = e_d if first else e_d + U * (mom * B).abs() + U * b.abs()
    e_p = abs(lr) * e_b + U * (lr * b).abs() + U * p_new.abs()
    return (p_new, b_out), (SECOND * e_p + TINY, SECOND * e_b + TINY), clip


MISTAKES_SGD = ('norm_unaveraged', 'wd_after_momentum', 'stale_first', 'tail_dropped')


def sgd_f32(p, g, buf, lr, mom, wd, gscale=1.0, max_norm=0.0, first=False):
    """The same step in plain f32 PyTorch (torch's own norm reduction)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    clip = f(1.0)
    if max_norm > 0:
        norm = torch.sqrt((g.float() * g.float()).sum()) * f(gscale)       # torch's f32 sum: cascaded, its own order
        clip = torch.clamp(f(max_norm) / (norm + f(1e-6)), max=1.0)
    d = g.float() * (f(gscale) * clip) + f(wd) * p.float()
    b = d if first else f(mom) * buf.float() + d
    return p.float() - f(lr) * b, b


def hvr_flat_numel():
    """Size of the flat parameter buffer dist_train.FlatParams builds for the HVR detector: its trainable parameters, every view
    padded to 64 elements (FlatParams' own rule, restated; the model is built on the host, nothing runs)."""
    import hvrnet_amd
    from hvrnet_amd import synthetic as S
    from hvrnet_amd.config import hvr_train_config
    model = hvrnet_amd.enable_training(hvrnet_amd.build_model(hvr_train_config(), S.synth_state_dict('hvr'), torch.float32, 'cpu'))
    return sum((p.numel() + 63) // 64 * 64 for p in model.parameters() if p.requires_grad)


def sgd_case(n, seed, stale=False):
    g_ = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) * 0.1
    buf = torch.randn(n, generator=g_) * (1e3 if stale else 0.05)
    return p, g, buf


def norm_f32_neighbours(g, gscale):
    """max_norm values equal to the averaged gradient's norm to within one f32 ulp: (one below, the nearest f32, one above)."""
    nrm = torch.tensor(math.sqrt(float((g.double() ** 2).sum())) * f32v(gscale) + f32v(1e-6), dtype=torch.float32)
    inf = torch.tensor(float('inf'))
    return float(torch.nextafter(nrm, -inf)), float(nrm), float(torch.nextafter(nrm, inf))


# ------------------------------------------------------------------------------------------------ relu_bwd, scale_rows
def relu_bwd_statement(dy, y):
    """dy where y > 0, else +0 (also where dy is NaN): exact in every dtype."""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def relu_case(n, dtype, seed):
    """y with +0, -0, the smallest positive subnormal of dtype, negative values; dy NaN on a share of the y <= 0 positions."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(n, generator=g).to(dtype)
    dy = torch.randn(n, generator=g).to(dtype)
    tiny = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}[dtype]
    y[0], y[1], y[2], y[3] = 0.0, -0.0, tiny, -tiny
    if n > 8:
        idx = torch.randperm(n, generator=g)[: max(4, n // 16)]
        y[idx[0::4]] = 0.0
        y[idx[1::4]] = -0.0
        y[idx[2::4]] = tiny
        y[idx[3::4]] = -tiny
    assert float(y[2]) > 0 and float(y[2]) == tiny
    nan_at = (y <= 0) & (torch.rand(n, generator=g) < 0.5)
    nan_at[0] = nan_at[1] = True
    dy[nan_at] = float('nan')
    return dy, y


def scale_rows_statement(w, s):
    """(w.float() * s[:, None]).to(dtype): the f32 product rounded to f32, then to the storage type (two roundings)."""
    R = w.shape[0]
    return (w.float().view(R, -1) * s.float().view(R, 1)).to(w.dtype).view(w.shape)


def scale_rows_single_rounding(w, s):
    """The mistake scale_rows must not make: the EXACT product rounded once to the storage type (a mixed-precision fma).  The exact
    product (35 bits at most: exact in f64) rounds like its f32 value except where that value is a tie of the storage type and the
    exact product is not: there the side the exact product lies on decides."""
    R = w.shape[0]
    exact = w.double().view(R, -1) * s.double().view(R, 1)
    p32 = exact.float()
    out = p32.to(w.dtype)
    if w.dtype != torch.float32:
        mant = {torch.bfloat16: 7, torch.float16: 10}[w.dtype]
        _, e = torch.frexp(p32)
        half_step = torch.pow(2.0, (e - 1 - mant - 1).float())
        fix = _is_tie(p32, w.dtype) & (exact != p32.double())
        side = torch.where(exact > p32.double(), p32 + half_step, p32 - half_step)     # the neighbour on the exact product's side
        out = torch.where(fix, side.to(w.dtype), out)
    return out.view(w.shape)


def scale_rows_case(R, C, dtype, seed):
    """w [R, C] in dtype, s [R] f32 -> (w, s, tie, inexact): `tie` marks products whose f32 value lies exactly half-way between two
    neighbours of dtype, `inexact` those whose f32 value is not the exact product.
    Rows 0, 4, 8, ... use s = 1.5 and rows 1, 5, ... s = 0.75: the product of a dtype value and 1.5 is exact in f32 and a tie for
    about half of all significands (ties-to-even is exercised in bulk).  The other rows have random 24-bit scales; there a product
    is a tie only when the f32 rounding of a 35-bit exact product happens to end in 1000...0 (2^-12 of all half values, 2^-16 of
    all bf16 values), so those are searched: for every such row all positive values of four binades of dtype are tried and the
    hits written into the row's first columns with alternating sign.  They are the inputs on which rounding the EXACT product
    once (a mixed-precision fma) and rounding twice can differ."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(R, generator=g) + 0.5).float()
    s[0::4] = 1.5
    s[1::4] = 0.75
    w = torch.randn((R, C), generator=g).to(dtype)
    if dtype != torch.float32:
        mant = {torch.bfloat16: 7, torch.float16: 10}[dtype]
        cand = torch.cat([(1 + torch.arange(2 ** mant).double() / 2 ** mant) * 2.0 ** e for e in (-2, -1, 0, 1)]).float()      # exact in dtype
        for r0 in range(0, R, 256):
            rows = torch.arange(r0, min(R, r0 + 256))
            prod = cand[None, :] * s[rows, None]
            hit = _is_tie(prod, dtype) & (prod.double() != cand.double()[None, :] * s[rows, None].double())
            for j, r in enumerate(rows.tolist()):
                v = cand[hit[j]][: C]
                if v.numel():
                    sign = torch.where(torch.arange(v.numel()) % 2 == 0, 1.0, -1.0)
                    w[r, : v.numel()] = (v * sign).to(dtype)
    prod = w.float() * s[:, None]
    return w, s, _is_tie(prod, dtype), prod.double() != w.double() * s.double()[:, None]


def _is_tie(x, dtype):
    """x f32: exactly half-way between two neighbouring values of dtype (normal range)."""
    if dtype == torch.float32:
        return torch.zeros_like(x, dtype=torch.bool)
    mant = {torch.bfloat16: 7, torch.float16: 10}[dtype]
    _, e = torch.frexp(x)
    half_step = torch.pow(2.0, (e - 1 - mant - 1).double())          # half the spacing of dtype at x
    q = x.double() / half_step
    return (q == q.round()) & (q.round().long() % 2 == 1) & (x != 0)


# ------------------------------------------------------------------------------------------------ case lists shared by both test files
def relation_cases():
    """(Mq, Mk, D, pad): the Mk edges (one key, around one block, % 4 != 0, 64 / 65 blocks) x Mq in {1, 37, 300} at D = 1 024 with
    Q / K alternately contiguous and sliced out of matrices 64 columns wider; the window size; the largest supported key count."""
    out = []
    for i, Mk in enumerate(RELATION_MK):
        for j, Mq in enumerate(RELATION_MQ):
            out.append((Mq, Mk, 1024, 64 * ((i + j) % 2)))
    out.append((4500, 4500, 1024, 0))
    out.append((8, MAX_KEYS, 64, 64))
    return out


def relation_scale(D):
    return 1.0 / math.sqrt(D)


def dscore_inputs(Mq, Mk, D, dtype, seed, device='cpu', cancel=False):
    """P [Mq, ldp] (a softmax over Mk columns, padding zero), dP like it, dO / O [Mq, D] as row slices of wider matrices, in
    dtype.  cancel: dP = delta + small noise, so that dP - delta cancels to ~2^-10 of its operands."""
    g = torch.Generator().manual_seed(seed)
    ldp = (Mk + 127) // 128 * 128
    P = torch.zeros((Mq, ldp))
    P[:, :Mk] = torch.softmax(torch.randn((Mq, Mk), generator=g) * 3, 1)
    dO = torch.randn((Mq, D + 64), generator=g).to(dtype).to(device)[:, :D]
    O = torch.randn((Mq, D + 32), generator=g).to(dtype).to(device)[:, :D]
    dP = torch.randn((Mq, ldp), generator=g)
    if cancel:
        delta = (dO.double() * O.double()).sum(1, keepdim=True).cpu()
        dP = (delta * (1 + 2.0 ** -10 * torch.randn((Mq, ldp), generator=g).double())).float()
    dP[:, Mk:] = 0
    return P.to(dtype).to(device), dP.to(dtype).to(device), dO, O


SGD_HYPER = dict(lr=5e-3, mom=0.9, wd=1e-4)


def sgd_configs(g, gscale):
    """(name, max_norm, first, stale) for a gradient g: no clipping (0), far above and far below the norm, and the norm itself to
    within one f32 ulp on both sides; first_step with a buffer of large stale values."""
    lo, mid, hi = norm_f32_neighbours(g, gscale)
    return [('noclip', 0.0, False, False), ('far_above', 1e3 * mid, False, False), ('far_below', 1e-3 * mid, False, False),
            ('ulp_below', lo, False, False), ('at_norm', mid, False, False), ('ulp_above', hi, False, False),
            ('first_stale', 1e-3 * mid, True, True), ('first_noclip', 0.0, True, True)]


SGD_SIZES = [1, 3, 4, 5, 1000003]
