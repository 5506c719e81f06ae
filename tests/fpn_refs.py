"""Statements for the multi-level feature path (hvrnet_amd/csrc/fpn.hip, hvrnet_amd/necks.py, SingleRoIExtractor at several levels).

  * fpn_forward: mmdet/models/necks/fpn.py:101-141 in f64 numpy (convs as sums over taps, nearest upsampling as index >> 1, the extra
    levels as a strided slice or stride-2 convs); `mistake` plants one wrong reading of it (MISTAKES).
  * level_rule: the level of a RoI as include/hvr_hip.h states it, float32 operation by operation; torch_levels: the reference's own
    expression (single_level.py:69-72).
  * merge_rule: what hvr_fpn_merge must write, evaluated by torch on the CPU: the f32 sum from the coarsest level inwards, rounded once.
  * roi_levels_statement: per level, the f64 interpolation matrix of tests/train_kernel_refs.py and its roi_forward_bound.
  * fpn_bound: the forward-error bound of the f32 FPN chain, computed from the fixture in f64.
The fixtures (tests/golden/g27_fpn.npz, fpn_modules.json) are written by tests/golden/make_fpn_golden.py, which runs the reference.
"""
import json
import os

import numpy as np
import torch

from tests import train_kernel_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
U = 2.0 ** -24
F32 = np.float32

IN_CHANNELS = [32, 64, 128, 256]
OUT_CHANNELS = 32
CONFIGS = dict(
    faster=dict(in_channels=IN_CHANNELS, out_channels=OUT_CHANNELS, num_outs=5),
    retina=dict(in_channels=IN_CHANNELS, out_channels=OUT_CHANNELS, start_level=1, add_extra_convs=True, num_outs=5),
    retina_outs=dict(in_channels=IN_CHANNELS, out_channels=OUT_CHANNELS, start_level=1, add_extra_convs=True, num_outs=5,
                     extra_convs_on_inputs=False, relu_before_extra_convs=True),
    relu3=dict(in_channels=IN_CHANNELS, out_channels=OUT_CHANNELS, end_level=3, num_outs=3, activation='relu'),
)
MISTAKES = ('bilinear', 'add_level_off', 'offset1', 'extra_on_outs')


def golden():
    return np.load(os.path.join(GOLDEN, 'g27_fpn.npz'))


def modules():
    with open(os.path.join(GOLDEN, 'fpn_modules.json')) as f:
        return json.load(f)


def fixture_inputs(g):
    return [g['x%d' % i] for i in range(len(IN_CHANNELS))]


def fixture_weights(g, name):
    pre = name + '.'
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre) and not k.startswith(pre + 'out')}


def fixture_outs(g, name):
    n = sum(1 for k in g.files if k.startswith(name + '.out'))
    return [g['%s.out%d' % (name, i)] for i in range(n)]


# ---- the FPN forward, f64 numpy ----
def conv2d(x, w, b, stride=1, pad=0, absolute=False):
    """x [B,C,H,W], w [O,C,KH,KW], b [O] -> [B,O,OH,OW] in f64, a sum over taps; absolute: |x| * |w| + |b|."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    if absolute:
        x, w, b = np.abs(x), np.abs(w), np.abs(b)
    B, C, H, W = x.shape
    O, _, KH, KW = w.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.zeros((B, O, OH, OW)) + b[None, :, None, None]
    for kh in range(KH):
        for kw in range(KW):
            patch = xp[:, :, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            out += np.einsum('bchw,oc->bohw', patch, w[:, :, kh, kw])
    return out


def up_nearest(x):
    return x.repeat(2, axis=2).repeat(2, axis=3)


def _lin2(x, axis):
    x = np.moveaxis(x, axis, -1)
    lo = np.concatenate([x[..., :1], x[..., :-1]], -1)
    hi = np.concatenate([x[..., 1:], x[..., -1:]], -1)
    out = np.stack([0.25 * lo + 0.75 * x, 0.75 * x + 0.25 * hi], -1).reshape(x.shape[:-1] + (2 * x.shape[-1],))
    return np.moveaxis(out, -1, axis)


def up_bilinear(x):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)"""
    return _lin2(_lin2(x, 2), 3)


def level_span(cfg):
    start, end = cfg.get('start_level', 0), cfg.get('end_level', -1)
    return start, (len(cfg['in_channels']) if end == -1 else end)


def fpn_forward(inputs, weights, cfg, mistake=None, absolute=False):
    """fpn.py:101-141 -> the list of output maps [B,C,H,W] f64.  absolute: the same chain on magnitudes (|x|, |w|, |b|, no ReLU gain):
    an upper bound on every partial magnitude, the scale of fpn_bound."""
    assert mistake is None or mistake in MISTAKES
    start, end = level_span(cfg)
    n = end - start
    relu = cfg.get('activation') == 'relu'
    act = (lambda v: np.maximum(v, 0.0)) if relu and not absolute else (lambda v: v)

    def conv(kind, i, x, **kw):
        return act(conv2d(x, weights['%s.%d.conv.weight' % (kind, i)], weights['%s.%d.conv.bias' % (kind, i)], absolute=absolute, **kw))
    lat = [conv('lateral_convs', i, inputs[i + start]) for i in range(n)]
    up = up_bilinear if mistake == 'bilinear' else up_nearest
    for i in range(n - 1, 0, -1):
        if mistake == 'add_level_off' and i >= 2:
            lat[i - 2] = lat[i - 2] + up(up(lat[i]))
        else:
            lat[i - 1] = lat[i - 1] + up(lat[i])
    outs = [conv('fpn_convs', i, lat[i], pad=1) for i in range(n)]
    num_outs = cfg['num_outs']
    if num_outs > n:
        if not cfg.get('add_extra_convs', False):
            o = 1 if mistake == 'offset1' else 0
            for _ in range(num_outs - n):
                outs.append(outs[-1][:, :, o::2, o::2])
        else:
            on_inputs = cfg.get('extra_convs_on_inputs', True)
            if on_inputs and mistake == 'extra_on_outs':
                cin = weights['fpn_convs.%d.conv.weight' % n].shape[1]
                src = np.concatenate([outs[-1], np.zeros((outs[-1].shape[0], cin - outs[-1].shape[1]) + outs[-1].shape[2:])], 1)
            else:
                src = inputs[end - 1] if on_inputs else outs[-1]
            outs.append(conv('fpn_convs', n, src, stride=2, pad=1))
            for i in range(n + 1, num_outs):
                src = outs[-1]
                if cfg.get('relu_before_extra_convs', False) and not absolute:
                    src = np.maximum(src, 0.0)
                outs.append(conv('fpn_convs', i, src, stride=2, pad=1))
    return outs


def rel_err(got, want):
    """max |got - want| / max |want| over a list of maps; a shape mismatch is infinite."""
    worst = 0.0
    for a, b in zip(got, want):
        if a.shape != b.shape:
            return float('inf')
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst if len(got) == len(want) else float('inf')


def fpn_bound(inputs, weights, cfg):
    """Per output map, the forward-error bound of the f32 chain against the f64 statement, from the fixture itself:
      a conv link with K products: (K + 3) u on the absolute-value conv of |x| and |w| plus |b| (K products and sums, the bias add and the
        store; the accumulation order is free), and an incoming error e reaches the output through |w|: conv(e, |w|);
      the merge: L u on the summed |lateral| of the chain (L - 1 f32 adds and the store), plus the laterals' own errors summed;
      the strided slice copies: exact.
    ReLU is 1-Lipschitz: bounds pass through it unchanged."""
    start, end = level_span(cfg)
    n = end - start
    W = lambda kind, i: np.abs(np.asarray(weights['%s.%d.conv.weight' % (kind, i)], np.float64))
    zb = lambda w: np.zeros(w.shape[0])

    def link(kind, i, x_abs, e_in, **kw):
        w = W(kind, i)
        K = w.shape[1] * w.shape[2] * w.shape[3]
        mag = conv2d(x_abs, w, np.abs(weights['%s.%d.conv.bias' % (kind, i)]), **kw)
        return mag, (K + 3) * U * mag + (conv2d(e_in, w, zb(w), **kw) if e_in is not None else 0.0)
    xs = [np.abs(np.asarray(x, np.float64)) for x in inputs]
    lat = [link('lateral_convs', i, xs[i + start], None) for i in range(n)]
    mag, err = [m for m, _ in lat], [e for _, e in lat]
    for i in range(n - 1, 0, -1):
        mag[i - 1] = mag[i - 1] + up_nearest(mag[i])
        err[i - 1] = err[i - 1] + up_nearest(err[i])
    err = [e + n * U * m for e, m in zip(err, mag)]
    outs = [link('fpn_convs', i, mag[i], err[i], pad=1) for i in range(n)]
    num_outs = cfg['num_outs']
    if num_outs > n:
        if not cfg.get('add_extra_convs', False):
            for _ in range(num_outs - n):
                outs.append((outs[-1][0][:, :, ::2, ::2], outs[-1][1][:, :, ::2, ::2]))
        else:
            src = (xs[end - 1], None) if cfg.get('extra_convs_on_inputs', True) else outs[-1]
            outs.append(link('fpn_convs', n, src[0], src[1], stride=2, pad=1))
            for i in range(n + 1, num_outs):
                outs.append(link('fpn_convs', i, outs[-1][0], outs[-1][1], stride=2, pad=1))
    return [e for _, e in outs]


# ---- the level of a RoI ----
def level_rule(rois, finest_scale, num_levels):
    """include/hvr_hip.h (hvr_roi_align_levels_fwd): float32, every operation rounded on its own; NaN fails every comparison."""
    r = np.asarray(rois, F32)
    with np.errstate(invalid='ignore'):
        w = (r[:, 3] - r[:, 1]).astype(F32) + F32(1)
        h = (r[:, 4] - r[:, 2]).astype(F32) + F32(1)
        s = np.sqrt((w * h).astype(F32)).astype(F32)
        v = (s / F32(finest_scale)).astype(F32) + F32(1e-6)
        lv = np.zeros(len(r), np.int32)
        for j in range(1, num_levels):
            lv += (v >= F32(2.0 ** j)).astype(np.int32)
    return lv


def torch_levels(rois, finest_scale, num_levels):
    """single_level.py:69-72 as written (float32 torch on the CPU)."""
    rois = torch.as_tensor(np.asarray(rois, F32))
    scale = torch.sqrt((rois[:, 3] - rois[:, 1] + 1) * (rois[:, 4] - rois[:, 2] + 1))
    lv = torch.floor(torch.log2(scale / finest_scale + 1e-6))
    return lv.clamp(min=0, max=num_levels - 1).long().numpy()


BOUNDARY_SIDES = [(56, 56), (112, 112), (224, 224), (448, 448), (112, 111), (111, 113), (224, 224), (223, 225)]


def boundary_boxes(x0=3.0, y0=5.0):
    """(x1, y1, x2, y2) of w x h boxes at the level boundaries of finest_scale = 56."""
    return np.array([[x0, y0, x0 + w - 1, y0 + h - 1] for w, h in BOUNDARY_SIDES], F32)


# ---- the merge kernel's rule, by torch on the CPU ----
def merge_rule(laterals):
    """laterals: CPU tensors [B,H_l,W_l,C] of one dtype -> the L - 1 maps hvr_fpn_merge writes: f32 sum from the top down, rounded once."""
    L = len(laterals)
    outs = []
    for l in range(L - 1):
        acc = laterals[L - 1].float()
        for j in range(L - 2, l - 1, -1):
            acc = laterals[j].float() + acc.repeat_interleave(2, 1).repeat_interleave(2, 2)
        outs.append(acc.to(laterals[0].dtype))
    return outs


# ---- RoIAlign behind the level select ----
def roi_levels_statement(rois, pool_rois, levels, feats, PH, PW, scales, sample_num):
    """feats: CPU f32/f64 [B,H_l,W_l,C] per level -> (ref, tol, nan) [K, PH*PW, C]: per level the interpolation matrix of
    train_kernel_refs and roi_forward_bound on the RoIs of that level; nan marks bins without samples (0 / 0)."""
    K, C = rois.shape[0], feats[0].shape[3]
    ref = torch.zeros((K, PH * PW, C), dtype=torch.float64)
    tol = torch.zeros_like(ref)
    nan = torch.zeros((K, PH * PW), dtype=torch.bool)
    levels = torch.as_tensor(np.asarray(levels)).long()
    for l, f in enumerate(feats):
        ks = torch.nonzero(levels == l).flatten()
        if ks.numel() == 0:
            continue
        B, H, W, _ = f.shape
        A = T.roi_align_matrix(pool_rois[ks], B, H, W, PH, PW, scales[l], sample_num)
        r, t = T.roi_forward_bound(A, f.reshape(-1, C).double())
        ref[ks], tol[ks] = r.view(-1, PH * PW, C), t.view(-1, PH * PW, C)
        dead = (A.sn_h == 0) | (A.sn_w == 0)
        nan[ks] = dead[:, None].expand(-1, PH * PW)
    return ref, tol, nan
