"""Plain float64 statements of the sigmoid focal loss kernels (hvrnet_amd/csrc/focal.hip; the rule: include/hvr_hip.h "Sigmoid focal
loss"), written independently of the HIP code, with the error bounds that tests/test_focal_refs.py (CPU) and tests/test_focal_gpu.py
(GPU) hold the kernels to: the elementwise loss and gradient, the reduced form, the RPN form, an f32 emulation of the stated forms, a
list of plausible mistakes, input families and a host restatement of the sampling-free anchor targets.

Error model and constants are those of tests/train_loss_refs.py (imported, not restated): u = 2^-24 per f32 operation, the library
functions' ulp limits, SECOND for the dropped products of errors, TINY per result that f32 flushes or rounds in its subnormal range.  A
sum whose longest chain of additions is c has error <= c u sum|term|.  No bound contains a value measured on a device.

The rule in the kernels' order, per element (x the logit, f32):
  e = expf(-|x|)                       relative 2 EXPF_ULP u  (+ TINY)
  L = log1pf(e)                        slope <= 1 in e: e 2 EXPF_ULP u + 2 LOG1PF_ULP u L
  lp = min(x,0) - L, lq = -max(x,0) - L          E_lp = E_L + u |lp|, E_lq likewise        (log p, log(1-p))
  r = 1 / (1 + e), er = e r;  p, q = (r, er) for x >= 0, (er, r) otherwise: relative (2 + 2 DIV_ULP + 4 EXPF_ULP) u =: rel_pq
  positive:  c = alpha expf(gamma lq),       l = c (-lp),   g = -(c (q - gamma p lp))
  negative:  c = (1-alpha) expf(gamma lp),   l = c (-lq),   g =   c (p - gamma q lq)
  the exponent gamma lz has error gamma E_lz + u |gamma lz|, which is the relative error of the power; expf adds 2 EXPF_ULP u; the
  coefficient two more roundings (1 - alpha and the product): rel_c.  l: rel_c + u on |l| plus c E_lz'.  The bracket s = q - gamma p lp
  (p - gamma q lq) is a sum of two NON-NEGATIVE terms: E_s = q rel_pq + gamma p |lp| (rel_pq + 2 u) + gamma p E_lp + u s.  g: rel_c + u on
  |g| plus c E_s.
"""
import math

import torch

from tests.train_loss_refs import (DIV_ULP, EXPF_ULP, LOG1PF_ULP, LOGF_ULP, SECOND, TINY, U, _smooth_l1, block_chain, f32v)  # noqa: F401

LOG_FLT_MIN = math.log(2.0 ** -126)        # the reference kernel's clamp on log p (x < -87.3)
REL_PQ = (2 + 2 * DIV_ULP + 4 * EXPF_ULP) * U

MISTAKES = ('alpha_swapped', 'gamma_on_own_prob', 'target_zero_based', 'negative_target_rows_counted', 'row_weight_ignored',
            'avg_pos_plus_neg', 'avg_unclamped', 'ignore_band_as_negative', 'grad_without_modulator_term', 'flt_min_clamp')


# ------------------------------------------------------------------------------------------------ elementwise rule
def focal_statement(x, t, gamma, alpha, mistake=None):
    """x [N, C] logits (any float type, taken exactly), t int64 [N] -> (dict(l, g), dict of bounds), [N, C] f64 each."""
    x = x.double()
    N, C = x.shape
    gamma, alpha = f32v(gamma), f32v(alpha)
    oma = 1.0 - alpha
    if mistake == 'alpha_swapped':
        alpha, oma = oma, alpha
    e = torch.exp(-x.abs())
    L = torch.log1p(e)
    lp, lq = x.clamp(max=0) - L, -x.clamp(min=0) - L
    if mistake == 'flt_min_clamp':
        lp, lq = lp.clamp(min=LOG_FLT_MIN), lq.clamp(min=LOG_FLT_MIN)
    r = 1 / (1 + e)
    p, q = torch.where(x >= 0, r, e * r), torch.where(x >= 0, e * r, r)
    cols = torch.arange(C, device=x.device)[None, :] + (0 if mistake == 'target_zero_based' else 1)
    pos = t[:, None] == cols
    live = torch.ones_like(t[:, None], dtype=torch.bool) if mistake == 'negative_target_rows_counted' else t[:, None] >= 0
    own = mistake == 'gamma_on_own_prob'
    # (log in the power, log in the product, the probability beside the modulator term, the other one) per element
    lz_m = torch.where(pos, lp if own else lq, lq if own else lp)
    lz_o, pa, pb = torch.where(pos, lp, lq), torch.where(pos, q, p), torch.where(pos, p, q)
    coef = torch.where(pos, torch.full_like(x, alpha), torch.full_like(x, oma))
    c = coef * torch.exp(gamma * lz_m)
    s = pa - gamma * pb * lz_o
    if mistake == 'grad_without_modulator_term':
        s = pa
    l = c * -lz_o
    g = torch.where(pos, -(c * s), c * s)
    livef = live.double()
    e_L = e * 2 * EXPF_ULP * U + TINY + 2 * LOG1PF_ULP * U * L
    e_m, e_o = e_L + U * lz_m.abs(), e_L + U * lz_o.abs()
    rel_c = gamma * e_m + U * (gamma * lz_m).abs() + 2 * EXPF_ULP * U + 2 * U
    b_l = SECOND * (l.abs() * (rel_c + U) + c * e_o) + TINY * (1 + lz_o.abs())
    e_s = pa * REL_PQ + gamma * pb * lz_o.abs() * (REL_PQ + 2 * U) + gamma * pb * e_o + U * s.abs() + 2 * TINY
    b_g = SECOND * (g.abs() * (rel_c + U) + c * e_s) + TINY * (1 + s.abs())
    return dict(l=l * livef, g=g * livef), dict(l=b_l * livef, g=b_g * livef)


def focal_bwd_statement(x, t, d_loss, gamma, alpha):
    """d_logits = dl/dx * d_loss: one more rounding."""
    ref, bound = focal_statement(x, t, gamma, alpha)
    d = ref['g'] * d_loss.double()
    return d, SECOND * (bound['g'] * d_loss.double().abs() + U * d.abs())


def focal_f32(x, t, gamma, alpha):
    """The stated forms evaluated by plain PyTorch in f32 on the CPU: an independent evaluation at the kernels' precision."""
    x = x.float().cpu()
    t = t.cpu()
    C = x.shape[1]
    gamma, alpha = torch.tensor(gamma, dtype=torch.float32), torch.tensor(alpha, dtype=torch.float32)
    e = torch.exp(-x.abs())
    L = torch.log1p(e)
    lp, lq = x.clamp(max=0) - L, -x.clamp(min=0) - L
    r = 1 / (1 + e)
    p, q = torch.where(x >= 0, r, e * r), torch.where(x >= 0, e * r, r)
    pos = t[:, None] == torch.arange(C)[None, :] + 1
    live = (t[:, None] >= 0).float()
    cp, cn = alpha * torch.exp(gamma * lq), (1 - alpha) * torch.exp(gamma * lp)
    l = torch.where(pos, cp * -lp, cn * -lq) * live
    g = torch.where(pos, -(cp * (q - gamma * p * lp)), cn * (p - gamma * q * lq)) * live
    return dict(l=l, g=g)


def focal_autograd_f64(x, t, gamma, alpha):
    """An independent torch-f64 autograd evaluation of BCEWithLogits x (alpha t + (1 - alpha)(1 - t)) pt^gamma (the formula of the
    reference's py_sigmoid_focal_loss), targets >= 0 only -> (l [N, C], d sum(l) / dx).  Written on cancellation-free primitives so
    that f64 autograd is good to 1e-12 at |x| = 20 as well: BCEWithLogits(x, t) = t softplus(-x) + (1 - t) softplus(x), and
    1 - sigmoid(x) = sigmoid(-x) (the literal `1 - pred.sigmoid()` and autograd's `sigmoid(x) - t` lose eight digits there)."""
    import torch.nn.functional as F
    xd = x.double().clone().requires_grad_(True)
    onehot = (t[:, None] == torch.arange(x.shape[1])[None, :] + 1).double()
    a = f32v(alpha)
    pt = torch.sigmoid(-xd) * onehot + torch.sigmoid(xd) * (1 - onehot)
    bce = F.softplus(-xd, threshold=700.0) * onehot + F.softplus(xd, threshold=700.0) * (1 - onehot)
    l = bce * (a * onehot + (1 - a) * (1 - onehot)) * pt.pow(f32v(gamma))
    g, = torch.autograd.grad(l.sum(), xd)
    return l.detach(), g


# ------------------------------------------------------------------------------------------------ reduced form
def focal_loss_splits(N, C):
    """hvr_focal_loss_splits restated (-> (S, rows per workgroup)): at least 2048 elements per workgroup, at most 2048 workgroups and at
    most one per row, consecutive rows, none empty."""
    if N <= 0 or C <= 0:
        return 0, 0
    s = max(1, min(-(-N * C // 2048), 2048, N))
    rows = -(-N // s)
    return -(-N // rows), rows


def focal_chain(N, C, ldl):
    """Longest chain of additions behind out1: a lane's steps (its rows of the workgroup's run, its pieces of a row, the elements of a
    piece; the larger of the 16-byte and the scalar mapping), six shuffle levels, four waves, then the merge of the S partials by one
    wave (ceil(S / 64) steps and six levels)."""
    S, rows = focal_loss_splits(N, C)
    steps = 0
    for V in ((1, 4) if ldl % 4 == 0 else (1,)):
        pieces = -(-ldl // V)
        G = min(256, pieces)
        R = 256 // G
        steps = max(steps, -(-rows // R) * -(-pieces // G) * V)
    return steps + 6 + 4 + -(-S // 64) + 6


def focal_loss_statement(x, C, t, w, gamma, alpha, loss_weight, avg, mistake=None):
    """hvr_focal_loss on x [N, ldl] (columns C .. ldl are pitch): -> (dict(out1 0-dim, d [N, ldl]), bounds).  avg: the divisor the kernel
    uses (the caller clamps a device count).  scale = loss_weight / avg is one f32 division; term w l one product; out1 = sum * scale."""
    N, ldl = x.shape
    ref, bound = focal_statement(x[:, :C], t, gamma, alpha, mistake=mistake)
    wd = torch.ones(N, dtype=torch.float64, device=x.device) if (w is None or mistake == 'row_weight_ignored') else w.double()
    scale = f32v(loss_weight) / f32v(avg)
    term = wd[:, None] * ref['l']
    e_term = wd.abs()[:, None] * bound['l'] + U * term.abs()
    out1 = term.sum() * scale
    b_out = SECOND * ((focal_chain(N, C, ldl) * U * term.abs().sum() + e_term.sum()) * abs(scale) + (1 + 2 * DIV_ULP) * U * out1.abs()) + TINY
    d = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    bd = torch.zeros_like(d)
    cw = scale * wd[:, None]
    d[:, :C] = cw * ref['g']
    bd[:, :C] = SECOND * (d[:, :C].abs() * (2 * DIV_ULP + 2) * U + cw.abs() * bound['g']) + TINY * (ref['g'] != 0).double()
    return dict(out1=out1, d=d), dict(out1=b_out, d=bd)


# ------------------------------------------------------------------------------------------------ RPN form
def rpn_focal_statement(o, A, labels, label_w, bbox_t, bbox_w, counts, beta, gamma, alpha, w_cls=1.0, w_bbox=1.0, mistake=None):
    """hvr_rpn_focal_loss on the fused head output o [rows, ldo]: -> (dict(out2, d_o), bounds).  M = rows A anchors, m = r A + a:
      loss_cls = (sum_m w_m l(x_m, label_m)) * (w_cls / avg),  loss_bbox = (sum_m sum_e smoothL1 bw) / avg * w_bbox,  avg = max(c0, 1)
      d_o = d(loss_cls + loss_bbox) / d o, zero elsewhere.  One workgroup of 1024: chain = ceil(M / 1024) + 10 (train_loss_refs).
    The smooth-L1 term and its gradient carry rpn_loss_statement's bounds and one more rounding for w_bbox."""
    rows, ldo = o.shape
    beta = f32v(beta)
    M = rows * A
    c0, c1 = int(counts[0]), int(counts[1])
    avg = float(max(c0, 1))
    if mistake == 'avg_pos_plus_neg':
        avg = float(max(c0, 1) + max(c1, 1))
    if mistake == 'avg_unclamped':
        avg = float(c0)
    x = o[:, :A].reshape(M, 1)
    t, w = labels.reshape(-1), label_w.double().reshape(-1)
    if mistake == 'ignore_band_as_negative':
        w = torch.where((w == 0) & (t == 0), torch.ones_like(w), w)
    if mistake == 'row_weight_ignored':
        w = torch.ones_like(w)
    ref, bound = focal_statement(x, t, gamma, alpha, mistake=mistake)
    l, g, b_l, b_g = ref['l'][:, 0], ref['g'][:, 0], bound['l'][:, 0], bound['g'][:, 0]
    wc, wb = f32v(w_cls), f32v(w_bbox)
    sc = wc / avg if avg else math.inf
    chain = block_chain(M, 1024, 10)
    term = w * l
    e_term = w.abs() * b_l + U * term.abs()
    loss_cls = term.sum() * sc
    b_cls = ((chain + 1 + 2 * DIV_ULP) * U * term.abs().sum() + e_term.sum()) * abs(sc)
    d = o[:, A:5 * A].double().reshape(M, 4) - bbox_t.double().reshape(M, 4)
    bw = bbox_w.double().reshape(M, 4)
    l1, dl1 = _smooth_l1(d, beta)
    tb = l1 * bw
    loss_bbox = tb.sum() / avg * wb if avg else tb.sum() * math.inf
    e_tb = bw.abs() * U * (d.abs() + (3 + 2 * DIV_ULP) * l1)
    b_bbox = ((chain + 2 + 2 * DIV_ULP) * U * tb.abs().sum() + e_tb.sum()) / max(avg, 1e-300) * abs(wb)
    dx = torch.zeros(o.shape, dtype=torch.float64, device=o.device)
    bd = torch.zeros_like(dx)
    cw = sc * w
    gc = cw * g
    dx[:, :A] = gc.view(rows, A)
    bd[:, :A] = (SECOND * (gc.abs() * (2 * DIV_ULP + 2) * U + cw.abs() * b_g) + TINY * (g != 0).double()).view(rows, A)
    cb = bw / max(avg, 1e-300) * wb
    gb = cb * dl1
    dx[:, A:5 * A] = gb.view(rows, 4 * A)
    bd[:, A:5 * A] = (SECOND * ((3 + 4 * DIV_ULP) * U * gb.abs() + 2 * U * cb.abs())).view(rows, 4 * A)
    return (dict(out2=torch.stack([loss_cls, loss_bbox]), d_o=dx),
            dict(out2=torch.stack([SECOND * b_cls + TINY, SECOND * b_bbox + TINY]), d_o=bd))


def rpn_focal_f32(o, A, labels, label_w, bbox_t, bbox_w, counts, beta, gamma, alpha, w_cls=1.0, w_bbox=1.0):
    """The RPN form by plain PyTorch in f32 (focal_f32 for the rule, another order of operations for the sums)."""
    rows = o.shape[0]
    M = rows * A
    of = o.float()
    avg = float(max(int(counts[0]), 1))
    f = focal_f32(of[:, :A].reshape(M, 1), labels.reshape(-1), gamma, alpha)
    w = label_w.float().reshape(-1)
    lc = (f['l'][:, 0] * w).sum() / avg * w_cls
    diff = of[:, A:5 * A].reshape(M, 4) - bbox_t.float().reshape(M, 4)
    b = torch.tensor(beta, dtype=torch.float32)
    ad = diff.abs()
    bwf = bbox_w.float().reshape(M, 4)
    lb = (torch.where(ad < b, 0.5 * ad * ad / b, ad - 0.5 * b) * bwf).sum() / avg * w_bbox
    d_o = torch.zeros_like(of)
    d_o[:, :A] = (f['g'][:, 0] * w / avg * w_cls).view(rows, A)
    d_o[:, A:5 * A] = (torch.where(ad < b, diff / b, torch.sign(diff)) * bwf / avg * w_bbox).view(rows, 4 * A)
    return dict(out2=torch.stack([lc, lb]), d_o=d_o)


# ------------------------------------------------------------------------------------------------ input families
EXTREME_VALUES = (0.0, 1e-4, -1e-4, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
FAMILIES = ('normal', 'extreme', 'saturated')


def logits_family(kind, N, ldl, seed, dtype=torch.float32):
    """normal: 4 x N(0, 1); extreme: drawn from EXTREME_VALUES (both sides of x = -87.3, where p underflows); saturated: all +-20."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'normal':
        x = torch.randn((N, ldl), generator=g) * 4.0
    elif kind == 'extreme':
        x = torch.tensor(EXTREME_VALUES)[torch.randint(0, len(EXTREME_VALUES), (N, ldl), generator=g)]
        x.view(-1)[:min(N * ldl, len(EXTREME_VALUES))] = torch.tensor(EXTREME_VALUES)[:min(N * ldl, len(EXTREME_VALUES))]
    else:
        assert kind == 'saturated'
        x = torch.where(torch.rand((N, ldl), generator=g) < 0.5, -20.0, 20.0)
    return x.to(dtype)


def targets_for(N, C, seed):
    """int64 [N] covering 0 (background), 1, C and -1 (nothing) as far as N allows, the rest uniform over -1 .. C."""
    g = torch.Generator().manual_seed(seed + 17)
    t = torch.randint(-1, C + 1, (N,), generator=g)
    for i, v in enumerate((1, 0, C, -1)):
        if i < N:
            t[(i * 5) % N if N > 4 else i] = v
    return t


def row_weights(N, seed):
    """f32 [N] in [0.5, 1.5) with exact zeros on about a fifth of the rows (and on row 0 when there are two rows or more)."""
    g = torch.Generator().manual_seed(seed + 29)
    w = 0.5 + torch.rand(N, generator=g)
    w[torch.rand(N, generator=g) < 0.2] = 0.0
    if N >= 2:
        w[0] = 0.0
    return w


def rpn_focal_case(H, W, A, ld, counts, seed, beta=1.0 / 9.0, family='normal'):
    """Input set of the RPN-form tests: c0 positives (label 1, weight 1, box weights 1), c1 negatives (label 0, weight 1) as far as they
    fit, the rest label 0 with weight 0 (ignore band / outside the image) except two anchors with label -1 and weight 1 (nothing).
    Box deltas: |pred - target| at least 1e-3 away from beta, so no element sits on the smooth-L1 kink."""
    g = torch.Generator().manual_seed(seed)
    rows = H * W
    M = rows * A
    o = torch.randn((rows, ld), generator=g) * 3.0
    o[:, :A] = logits_family(family, rows, A, seed + 1)
    labels = torch.zeros(M, dtype=torch.long)
    label_w = torch.zeros(M)
    bbox_w = torch.zeros((M, 4))
    perm = torch.randperm(M, generator=g)
    c0, c1 = min(counts[0], M // 2), min(counts[1], M - M // 2)
    labels[perm[:c0]] = 1
    label_w[perm[:c0 + c1]] = 1.0
    bbox_w[perm[:c0]] = 1.0
    rest = perm[c0 + c1:]
    if rest.numel() >= 4:
        labels[rest[:2]] = -1
        label_w[rest[:2]] = 1.0
    bbox_t = torch.randn((M, 4), generator=g)
    d = o[:, A:5 * A].reshape(M, 4) - bbox_t
    b32 = float(torch.tensor(beta, dtype=torch.float32))
    near = (d.abs() - b32).abs() < 2e-3
    bbox_t = torch.where(near, bbox_t - 0.01 * torch.sign(d + (d == 0).float()), bbox_t)
    d = o[:, A:5 * A].reshape(M, 4) - bbox_t
    assert bool(((d.abs().double() - b32).abs() >= 1e-3).all())
    return dict(o=o, A=A, labels=labels, label_w=label_w, bbox_t=bbox_t, bbox_w=bbox_w, counts=torch.tensor((c0, c1), dtype=torch.int32), beta=beta)


# ------------------------------------------------------------------------------------------------ sampling-free anchor targets
# train_cfg.rpn of the anchor-target case of tests/golden/focal.npz (tests/golden/make_focal_golden.py imports it; the tests must not import the
# maker, whose loader pins the CPU numeric path for the whole process)
AT_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, ignore_iof_thr=-1),
              sampler=dict(type='RandomSampler', num=8, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),     # ignored: sampling=False
              allowed_border=0, pos_weight=-1, debug=False)


def anchor_target_host(anchors, valid, gts, img_shape, cfg, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """anchor_target_single(..., sampling=False, gt_labels=None, unmap_outputs=True) restated on the host in f32 (anchor_target.py:92-155
    with max_iou_assigner.py:48-173, geometry.py:46-60, transforms.py:6-31): every anchor inside the image is assigned; positives label 1,
    weight 1 (pos_weight <= 0), box targets and box weights 1; negatives weight 1; the ignore band and the anchors outside the image
    weight 0.  -> (labels, label_weights, bbox_targets, bbox_weights, (#pos, #neg))."""
    a, gt = anchors.float().cpu(), gts.float().cpu()
    n = a.shape[0]
    h, w = img_shape[:2]
    border = cfg['allowed_border']
    inside = torch.ones(n, dtype=torch.bool) if valid is None else valid.cpu().bool()
    if border >= 0:
        inside = inside & (a[:, 0] >= -border) & (a[:, 1] >= -border) & (a[:, 2] < w + border) & (a[:, 3] < h + border)
    asg = cfg['assigner']
    lt, rb = torch.max(gt[:, None, :2], a[None, :, :2]), torch.min(gt[:, None, 2:], a[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    area_g, area_a = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1), (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    iou = overlap / (area_g[:, None] + area_a[None, :] - overlap)                   # [k, n]
    iou_in = torch.where(inside[None, :], iou, torch.full_like(iou, -1.0))
    max_ov, arg = iou_in.max(0)
    gt_max = iou_in.max(1).values
    gt_inds = torch.full((n,), -1, dtype=torch.long)
    gt_inds[inside & (max_ov >= 0) & (max_ov < asg['neg_iou_thr'])] = 0
    posm = inside & (max_ov >= asg['pos_iou_thr'])
    gt_inds[posm] = arg[posm] + 1
    for i in range(gt.shape[0]):
        if gt_max[i] >= asg['min_pos_iou']:
            gt_inds[inside & (iou_in[i] == gt_max[i])] = i + 1
    labels = torch.zeros(n, dtype=torch.long)
    label_w = torch.zeros(n)
    bbox_t, bbox_w = torch.zeros((n, 4)), torch.zeros((n, 4))
    pos, neg = gt_inds > 0, gt_inds == 0
    labels[pos] = 1
    label_w[pos] = 1.0 if cfg['pos_weight'] <= 0 else cfg['pos_weight']
    label_w[neg] = 1.0
    pa, pg = a[pos], gt[gt_inds[pos] - 1]
    px, py, pw, ph = (pa[:, 0] + pa[:, 2]) * 0.5, (pa[:, 1] + pa[:, 3]) * 0.5, pa[:, 2] - pa[:, 0] + 1, pa[:, 3] - pa[:, 1] + 1
    gx, gy, gw, gh = (pg[:, 0] + pg[:, 2]) * 0.5, (pg[:, 1] + pg[:, 3]) * 0.5, pg[:, 2] - pg[:, 0] + 1, pg[:, 3] - pg[:, 1] + 1
    deltas = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], 1)
    bbox_t[pos] = (deltas - torch.tensor(means)[None, :]) / torch.tensor(stds)[None, :]
    bbox_w[pos] = 1.0
    return labels, label_w, bbox_t, bbox_w, (int(pos.sum()), int(neg.sum()))
