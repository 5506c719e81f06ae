"""Plain float64 statements (numpy) of the Guided Anchoring RPN kernels -- hvr_ga_mask_offsets, hvr_masked_conv_fwd,
hvr_ga_rpn_proposals -- and of GARPNHead's forward chain, written from the rules include/hvr_hip.h states (which follow
mmdet/models/anchor_heads/guided_anchor_head.py:197-208,326-362, ga_rpn_head.py:60-127, mmdet/ops/masked_conv/masked_conv.py:15-53 and
mmdet/core/bbox/transforms.py:78-110), independently of the HIP code, with the error bounds tests/test_ga_rpn_refs.py (CPU, against the
reference's own results in tests/golden/g26_ga_rpn.npz) and tests/test_ga_rpn_gpu.py hold the kernels to.

Bounds (u = 2^-24, first order, times SECOND; no bound contains a value measured on the device):
  sigmoid   1 / (1 + expf(-x)): expf within EXPF_ULP ulp = 2 EXPF_ULP u (the OpenCL full-profile limit, as everywhere in this suite:
            train_loss_refs.py), damped by e / (1 + e) <= 1, then a correctly rounded add and divide: S_SIGMOID = 2 EXPF_ULP + 2 units of u,
            relative to the result.
  mask      exact wherever |sigmoid(loc) - f32(thr)| exceeds that bound; pixels inside it are `ambiguous` (either answer follows the rule
            in f32).  The threshold is the f32 value of loc_filter_thr.  loc == 0 at thr == 0.5 is exact in any arithmetic (1 / (1 + 1)).
  offsets   w0 s0 + w1 s1: each term is rounded as a product and passes one addition: 2 u (|w0 s0| + |w1 s1|).
  masked conv  operands are the stored values of the mode (the statement reads them as they are stored: no operand rounding is left
            to bound); K = KH KW Cin fused multiply-adds and the wave's butterfly in SOME fixed order, then the bias: a term passes
            through at most K additions whatever the association: (K + 1) u (sum |x| |w| + |bias|).  Unkept pixels: exactly 0.
  boxes     every f32 operation of the two delta2bbox steps rounded on its own (the file is built with -ffp-contract=off): the error is
            carried through the formulas operation by operation (`delta2bbox_err`): u |result| per operation, expf as above, the
            incoming error of the guided anchor through the second step's derivatives.  With shape deltas at the 1e-6 clip an anchor
            is ~1e8 px wide and its f32 coordinates carry several px: the bound says so, and the image clip removes it.
The forward chain: `forward_chain_statement` evaluates the whole head in f64 from the input map to the four outputs (the deformable conv
through dcn_refs.sampler_statement).  It carries NO end-to-end bound: the mask is a threshold and the sampler's corner set changes where
an offset crosses a cell border, so an error of the stage before is not carried through by a derivative.  The GPU test therefore holds
every LINK to its own statement and bound on the stored values the device produced for the link before (conv_statement /
gemm_statement and the mfma bound of forward_kernel_refs.py for the convs, the sampler's, and the ones above), and the head's outputs
to the chain of those links bit for bit; the f64 chain is checked on the CPU against torch's own convs where the offsets are zero.

`mistake=`: plausible mistakes stated exactly (MISTAKES); tests/test_ga_rpn_refs.py shows that each one fails.
"""
import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
EXPF_ULP = 3.0
S_SIGMOID = 2 * EXPF_ULP + 2
ANCHORING_CLIP = 1e-6
WH_RATIO_CLIP = 16 / 1000

MISTAKES = ('bias_at_unkept', 'frame0_mask', 'gt_threshold', 'anchoring_clip_16_1000', 'anchoring_means_skip_xy', 'dw_dh_swapped',
            'square_ratio', 'square_scale', 'topk_unfiltered', 'no_img_clip', 'nms_post_after_max_num')
MASK_MISTAKES = ('gt_threshold', )
CONV_MISTAKES = ('bias_at_unkept', 'frame0_mask')
ANCHOR_MISTAKES = ('anchoring_clip_16_1000', 'anchoring_means_skip_xy', 'dw_dh_swapped', 'square_ratio', 'square_scale')
READOUT_MISTAKES = ('topk_unfiltered', 'no_img_clip', 'nms_post_after_max_num')


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-x))


def sigmoid_bound(s):
    return SECOND * S_SIGMOID * U * np.abs(s)


# ------------------------------------------------------------------------------------------------ mask, offsets
def loc_mask_statement(loc, thr, mistake=None):
    """loc [...] logits (f32 values) -> (keep bool, ambiguous bool): keep = sigmoid(loc) >= f32(thr)."""
    s = sigmoid(loc)
    t = float(np.float32(thr))
    keep = (s > t) if mistake == 'gt_threshold' else (s >= t)
    exact = (np.asarray(loc) == 0.0) & (t == 0.5)
    return keep, (np.abs(s - t) <= sigmoid_bound(s)) & ~exact


def offsets_statement(shape, w_off):
    """shape [..., 2], w_off [nch, 2] -> (om [..., nch], bound)."""
    shape, w_off = np.asarray(shape, np.float64), np.asarray(w_off, np.float64)
    a, b = shape[..., 0:1] * w_off[:, 0], shape[..., 1:2] * w_off[:, 1]
    return a + b, SECOND * 2 * U * (np.abs(a) + np.abs(b))


# ------------------------------------------------------------------------------------------------ masked conv
def masked_conv_statement(x, w, bias, keep, pad, mistake=None):
    """x [B,H,W,Cin], w [Cout,KH,KW,Cin], bias [Cout] or None, keep [B,H,W] -> (out [B,H,W,Cout], bound): bias + conv at the kept pixels,
    0 at the others.  Mistakes: 'bias_at_unkept' (an unkept pixel gets the bias), 'frame0_mask' (frame 0's mask for every frame)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    keep = np.asarray(keep).astype(bool)
    if mistake == 'frame0_mask':
        keep = np.broadcast_to(keep[0:1], keep.shape)
    bz = np.zeros(Cout) if bias is None else np.asarray(bias, np.float64)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    acc, mag = np.zeros((B, H, W, Cout)), np.zeros((B, H, W, Cout))
    for kh in range(KH):
        for kw in range(KW):
            v = xp[:, kh:kh + H, kw:kw + W]
            acc += v @ w[:, kh, kw].T
            mag += np.abs(v) @ np.abs(w[:, kh, kw]).T
    out = np.where(keep[..., None], acc + bz, bz if mistake == 'bias_at_unkept' else 0.0)
    bound = np.where(keep[..., None], SECOND * (KH * KW * Cin + 1) * U * (mag + np.abs(bz)), 0.0)
    return out, bound


def forward_chain_statement(x, prm, thr, dg):
    """GARPNHead.forward in f64 (guided_anchor_head.py:197-208 behind ga_rpn_head.py:28-33).  x [B,H,W,C]; prm: rpn_conv (w [C,3,3,C], b),
    loc (w [1,1,1,C], b), shape (w [2,1,1,C], b), off [dg 18, 2], adapt w [C,3,3,C], cls (w [1,1,1,C], b), reg (w [4,1,1,C], b), all in
    the packed [Cout,KH,KW,Cin] layout -> dict(y, loc [B,H,W], shape [B,H,W,2], keep, om, z, cls [B,H,W], reg [B,H,W,4])."""
    import torch
    from tests import dcn_refs as D
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    everywhere = np.ones((B, H, W), bool)
    y = np.maximum(masked_conv_statement(x, prm['rpn_conv'][0], prm['rpn_conv'][1], everywhere, 1)[0], 0.0)
    loc = masked_conv_statement(y, prm['loc'][0], prm['loc'][1], everywhere, 0)[0][..., 0]
    shape = masked_conv_statement(y, prm['shape'][0], prm['shape'][1], everywhere, 0)[0]
    keep = loc_mask_statement(loc, thr)[0]
    om = offsets_statement(shape, prm['off'])[0]
    col = D.sampler_statement(torch.from_numpy(y), torch.from_numpy(om).float(), 3, 3, 1, 1, 1, dg, False)[0].numpy()
    z = np.maximum(col @ np.asarray(prm['adapt'], np.float64).reshape(C, -1).T, 0.0).reshape(B, H, W, -1)
    cls = masked_conv_statement(z, prm['cls'][0], prm['cls'][1], keep, 0)[0][..., 0]
    reg = masked_conv_statement(z, prm['reg'][0], prm['reg'][1], keep, 0)[0]
    return dict(y=y, loc=loc, shape=shape, keep=keep, om=om, z=z, cls=cls, reg=reg)


# ------------------------------------------------------------------------------------------------ anchors, boxes
def base_square(base_size, scale, ratio=1.0):
    """AnchorGenerator(base_size, [scale], [ratio]).base_anchors[0] (anchor_generator.py:22-46, scale_major, ctr = (base_size - 1) / 2)."""
    w = h = float(base_size)
    ctr = 0.5 * (w - 1)
    hr = np.sqrt(ratio)
    ws, hs = w * (1 / hr) * scale, h * hr * scale
    return np.round(np.array([ctr - 0.5 * (ws - 1), ctr - 0.5 * (hs - 1), ctr + 0.5 * (ws - 1), ctr + 0.5 * (hs - 1)]))


def grid_squares(base, H, W, stride):
    ys, xs = np.meshgrid(np.arange(H) * stride, np.arange(W) * stride, indexing='ij')
    shift = np.stack([xs, ys, xs, ys], -1).reshape(-1, 4).astype(np.float64)
    return shift + np.asarray(base, np.float64)[None]


def delta2bbox_err(box, ebox, d, means, stds, clip, max_shape=None, swap_wh=False):
    """delta2bbox (transforms.py:78-110) in f64 with the bound on the f32 evaluation carried along.  box [n,4] with incoming error ebox
    [n,4] (0 for exact inputs), d [n,4] f32-exact deltas -> (out [n,4], eout [n,4])."""
    box, ebox, d = np.asarray(box, np.float64), np.asarray(ebox, np.float64), np.asarray(d, np.float64)
    m, s = np.asarray(means, np.float64), np.asarray(stds, np.float64)
    dn = d * s + m
    edn = U * (np.abs(d * s) + np.abs(dn))
    if swap_wh:
        dn, edn = dn[:, [0, 1, 3, 2]], edn[:, [0, 1, 3, 2]]
    mr = abs(np.log(clip))
    out, eout = np.zeros_like(box), np.zeros_like(box)
    for ax in (0, 1):
        a1, a2, e1, e2 = box[:, ax], box[:, ax + 2], ebox[:, ax], ebox[:, ax + 2]
        dc, edc = dn[:, ax], edn[:, ax]
        ds, eds = np.clip(dn[:, ax + 2], -mr, mr), edn[:, ax + 2]
        p = (a1 + a2) * 0.5
        ep = 0.5 * (e1 + e2) + U * (np.abs(a1 + a2) * 0.5 + np.abs(p))
        pw = a2 - a1 + 1.0
        epw = e1 + e2 + U * (np.abs(a2 - a1) + np.abs(pw))
        ex = np.exp(ds)
        g = pw * ex
        eg = epw * ex + np.abs(g) * (eds + 2 * EXPF_ULP * U) + U * np.abs(g)
        c = p + pw * dc
        ec = ep + epw * np.abs(dc) + np.abs(pw) * edc + U * np.abs(pw * dc) + U * np.abs(c)
        lo, hi = c - g * 0.5 + 0.5, c + g * 0.5 - 0.5
        elo = ec + 0.5 * eg + U * (np.abs(c - g * 0.5) + np.abs(lo))
        ehi = ec + 0.5 * eg + U * (np.abs(c + g * 0.5) + np.abs(hi))
        if max_shape is not None:
            top = max_shape[1 - ax] - 1.0      # x: img_w - 1, y: img_h - 1
            lo, hi = np.clip(lo, 0.0, top), np.clip(hi, 0.0, top)
        out[:, ax], out[:, ax + 2], eout[:, ax], eout[:, ax + 2] = lo, hi, elo, ehi
    return out, SECOND * eout


def guided_anchors_statement(shape, keep, base, stride, means, stds, mistake=None, octave_base_scale=8, base_size=None):
    """shape [H,W,2], keep [H,W] -> (anchors [n,4] of the kept pixels in row-major order, their bound, the kept pixel indices).
    Mistakes: the clip 16 / 1000 instead of 1e-6, the means left off dx / dy, dw and dh swapped, a square of ratio 2 or of the second octave
    scale."""
    H, W, _ = shape.shape
    if mistake in ('square_ratio', 'square_scale'):
        bs = float(stride if base_size is None else base_size)
        base = base_square(bs, octave_base_scale, 2.0) if mistake == 'square_ratio' else base_square(bs, octave_base_scale * 2 ** (1 / 3.0))
    idx = np.flatnonzero(np.asarray(keep).reshape(-1))
    sq = grid_squares(base, H, W, stride)[idx]
    d = np.zeros((len(idx), 4))
    d[:, 2:] = np.asarray(shape, np.float64).reshape(-1, 2)[idx]
    means = np.asarray(means, np.float64).copy()
    if mistake == 'anchoring_means_skip_xy':
        means[:2] = 0.0
    clip = WH_RATIO_CLIP if mistake == 'anchoring_clip_16_1000' else ANCHORING_CLIP
    an, ean = delta2bbox_err(sq, np.zeros_like(sq), d, means, stds, clip, None, swap_wh=mistake == 'dw_dh_swapped')
    return an, ean, idx


def iou_plus1(a, b):
    """IoU of box a [4] with boxes b [n,4], the "+1" pixel convention (nms_cpu.cpp:18,46-54)."""
    xx1, yy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xx2, yy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.maximum(0.0, xx2 - xx1 + 1) * np.maximum(0.0, yy2 - yy1 + 1)
    aa = (a[2] - a[0] + 1) * (a[3] - a[1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return inter / (aa + ab - inter)


def greedy_nms(boxes, scores, thr):
    """Survivors in score order (stable: lower index first on equal scores); IoU >= thr suppresses."""
    order = np.argsort(-scores, kind='stable')
    alive = np.ones(len(order), bool)
    kept = []
    for oi, i in enumerate(order):
        if not alive[oi]:
            continue
        kept.append(i)
        rest = order[oi + 1:]
        alive[oi + 1:] &= ~(iou_plus1(boxes[i], boxes[rest]) >= thr)
    return np.array(kept, dtype=np.int64)


def proposals_statement(cls, reg, shape, keep, base, stride, anchoring_means, anchoring_stds, target_means, target_stds, img_shape, nms_pre,
                        nms_post, max_num, nms_thr, mistake=None, wh_ratio_clip=WH_RATIO_CLIP):
    """One frame: cls [H,W], reg [H,W,4], shape [H,W,2], keep [H,W] -> dict(props [n,5], bound [n,4], pixels [n] (the pixel of every
    proposal), cand (candidate pixels after the top-k, score order), cand_boxes, cand_scores).  No kept pixel: n = 0.
    Mistakes: 'topk_unfiltered' (the top nms_pre taken over all pixels, the mask applied afterwards), 'no_img_clip',
    'nms_post_after_max_num' (of the survivors the top max_num by score first, then the first nms_post of those in list order)."""
    am = mistake if mistake in ANCHOR_MISTAKES else None
    H, W = cls.shape
    keepf = np.asarray(keep).reshape(-1).astype(bool)
    score_all = sigmoid(np.asarray(cls, np.float64).reshape(-1))
    an, ean, idx = guided_anchors_statement(shape, keep, base, stride, anchoring_means, anchoring_stds, am)
    empty = dict(props=np.zeros((0, 5)), bound=np.zeros((0, 4)), pixels=np.zeros(0, np.int64), cand=np.zeros(0, np.int64),
                 cand_boxes=np.zeros((0, 4)), cand_scores=np.zeros(0))
    if len(idx) == 0:
        return empty
    sc = score_all[idx]
    sel = np.arange(len(idx))
    if mistake == 'topk_unfiltered':
        if nms_pre > 0 and len(score_all) > nms_pre:
            top = np.argsort(-score_all, kind='stable')[:nms_pre]
            pos = {p: i for i, p in enumerate(idx)}
            sel = np.array([pos[p] for p in top if keepf[p]], dtype=np.int64)
        if len(sel) == 0:
            return empty
    elif nms_pre > 0 and len(idx) > nms_pre:
        sel = np.argsort(-sc, kind='stable')[:nms_pre]
    d = np.asarray(reg, np.float64).reshape(-1, 4)[idx[sel]]
    boxes, eb = delta2bbox_err(an[sel], ean[sel], d, target_means, target_stds, wh_ratio_clip,
                               None if mistake == 'no_img_clip' else img_shape)
    s = sc[sel]
    # the survivors in the order of the candidate list `sel`: score order behind a top-k, row-major without one (the reference's CPU NMS
    # returns them by ascending input index, nms_cpu.cpp:68-70)
    k = np.sort(greedy_nms(boxes, s, nms_thr))
    if mistake == 'nms_post_after_max_num':
        k = np.sort(k[np.argsort(-s[k], kind='stable')[:max_num]])[:nms_post]
    else:
        k = k[:nms_post]
    k = k[np.argsort(-s[k], kind='stable')[:min(max_num, len(k))]]
    so = np.argsort(-s, kind='stable')
    return dict(props=np.concatenate([boxes[k], s[k, None]], 1), bound=eb[k], pixels=idx[sel][k], cand=idx[sel][so], cand_boxes=boxes[so],
                cand_scores=s[so])


def readout_conditions(r, nms_thr, iou_margin=1e-5):
    """The conditions under which the SELECTION of proposals_statement is forced in f32 too, on the statement alone: candidate scores
    distinct by more than their bounds, no candidate pair with an IoU within iou_margin of nms_thr.  -> (scores_distinct, iou_clear)."""
    s, b = r['cand_scores'], r['cand_boxes']
    ok_s = True
    if len(s) > 1:
        gap = s[:-1] - s[1:]
        ok_s = bool((gap > sigmoid_bound(s[:-1]) + sigmoid_bound(s[1:])).all())
    ok_i = True
    for i in range(len(b) - 1):
        ok_i = ok_i and bool((np.abs(iou_plus1(b[i], b[i + 1:]) - nms_thr) > iou_margin).all())
    return ok_s, ok_i


# ------------------------------------------------------------------------------------------------ planted-mistake dispatch
def differs(a, b):
    """Two read-outs differ in selection (count, pixels) or in a box by more than both bounds together."""
    if len(a['pixels']) != len(b['pixels']) or (a['pixels'] != b['pixels']).any():
        return True
    return bool((np.abs(a['props'][:, :4] - b['props'][:, :4]) > a['bound'] + b['bound'] + 1e-9).any())
