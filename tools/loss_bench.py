"""Cost of the regression / IoU / GHM loss kernels (csrc/reg_loss.hip, csrc/ghm.hip) on an otherwise idle MI355X, in one process,
HIP-event times (warm-up, then the median of --iters groups of back-to-back launches; the calls compared at one shape take turns
group by group -- tools/gconv_bench.py's method):

  reduced  every reduced form (loss and gradient in one call) at RPN scale, 38 x 63 x 12 anchors x 4, beside (a) the same rule written
           as a composite of torch ops on the device, forward + backward through autograd, and (b) the project's own copy of the bytes
           the kernel moves (native.avgpool_nhwc(x, 1) over a map of that many bytes).  Ratios composite / kernel and kernel / copy are
           printed; a form slower than its composite says so.
  ghm      hvr_ghmc_loss at 150000 x 80 (the size the focal bench used) and at RPN scale, hvr_ghmr_loss at RPN scale, beside the
           composite of ghm_loss.py WITHOUT its per-bin .item() loop (bucketize + bincount on the device) and the copy.
  train    one SELSA training iteration (forward + backward, T = 3, 608 x 1008, the built-in training config without OHEM) with
           loss_bbox = BalancedL1Loss in both heads beside SmoothL1Loss, alternating --reps times.  --no-train skips it.

    python tools/loss_bench.py [--iters 30] [--out profiles/loss_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, synthetic as S  # noqa: E402
from hvrnet_amd.config import selsa_train_config  # noqa: E402
from tools.gconv_bench import DEV, Report, timed  # noqa: E402

RPN_N = 38 * 63 * 12


def copy_of(nbytes):
    """The project's own copy of `nbytes` bytes read and as many written: a 1 x 1 average pool of an f32 NHWC map."""
    x = torch.zeros((1, 1, max(nbytes // 2 // 4 // 64, 1), 64), device=DEV)
    return lambda i: native.avgpool_nhwc(x, 1)


def smooth_l1_c(p, t, beta=1.0 / 9.0):
    d = (p - t).abs()
    return torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)


def balanced_l1_c(p, t, beta=1.0, alpha=0.5, gamma=1.5):
    d = (p - t).abs()
    b = math.e ** (gamma / alpha) - 1
    return torch.where(d < beta, alpha / b * (b * d + 1) * torch.log(b * d / beta + 1) - alpha * d, gamma * d + gamma / b - alpha * beta)


def mse_c(p, t):
    return (p - t) ** 2


def iou_c(p, t, eps=1e-6):
    lt, rb = torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    a1, a2 = (p[:, 2] - p[:, 0] + 1) * (p[:, 3] - p[:, 1] + 1), (t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1)
    return -(ov / (a1 + a2 - ov)).clamp(min=eps).log()


def bounded_iou_c(p, t, beta=0.2, eps=1e-3):
    pcx, pcy, pw, ph = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5, p[:, 2] - p[:, 0] + 1, p[:, 3] - p[:, 1] + 1
    tcx, tcy, tw, th = (t[:, 0] + t[:, 2]) * 0.5, (t[:, 1] + t[:, 3]) * 0.5, t[:, 2] - t[:, 0] + 1, t[:, 3] - t[:, 1] + 1
    dx, dy = tcx - pcx, tcy - pcy
    ldx = 1 - torch.max((tw - 2 * dx.abs()) / (tw + 2 * dx.abs() + eps), torch.zeros_like(dx))
    ldy = 1 - torch.max((th - 2 * dy.abs()) / (th + 2 * dy.abs() + eps), torch.zeros_like(dy))
    ldw = 1 - torch.min(tw / (pw + eps), pw / (tw + eps))
    ldh = 1 - torch.min(th / (ph + eps), ph / (th + eps))
    c = torch.stack([ldx, ldy, ldw, ldh], -1)
    return torch.where(c < beta, 0.5 * c * c / beta, c - 0.5 * beta)


def composite(fn, p, t, w, avg):
    def run(i):
        x = p.detach().requires_grad_(True)
        ((fn(x, t) * w).sum() / avg).backward()
        return x.grad
    return run


def ghm_c(kind, edges, mu=0.02):
    """ghm_loss.py without the per-bin .item() loop: bucketize + bincount on the device, momentum 0."""
    bins = edges.numel() - 1

    def run(p, t, w):
        x = p.detach().requires_grad_(True)
        if kind == 'ghmc':
            g = (x.sigmoid().detach() - t).abs()
        else:
            d = x - t
            r = torch.sqrt(d * d + mu * mu)
            g = (d / r).abs().detach()
        valid = w > 0
        tot = (valid.float().sum() if kind == 'ghmc' else w.sum()).clamp(min=1.0)
        idx = (torch.bucketize(g, edges, right=True) - 1).clamp(0, bins - 1)
        cnt = torch.bincount(idx[valid], minlength=bins).float()
        n = (cnt > 0).sum().clamp(min=1)
        wb = torch.where(cnt > 0, tot / cnt.clamp(min=1) / n, torch.zeros_like(cnt))[idx] * valid
        loss = (F.binary_cross_entropy_with_logits(x, t, wb, reduction='sum') if kind == 'ghmc' else ((r - mu) * wb).sum()) / tot
        loss.backward()
        return x.grad
    return run


def line_of(name, shape, res, lines, js):
    k, c, cp = res
    verdict = 'faster than' if c[0] > k[0] else 'SLOWER than'
    lines.append('  %-22s %-12s kernel %8.1f us (%.1f, %.1f)   composite %8.1f us (%.1f, %.1f)   copy %7.1f us   composite / kernel %5.2f (%s its composite)   kernel / copy %5.2f'
                 % (name, shape, k[0], k[1], k[2], c[0], c[1], c[2], cp[0], c[0] / k[0], verdict, k[0] / cp[0]))
    js['%s %s' % (name, shape)] = dict(kernel_us=k[0], composite_us=c[0], copy_us=cp[0], composite_over_kernel=c[0] / k[0], kernel_over_copy=k[0] / cp[0])


def reduced_report(args, lines, js):
    lines.append('reduced forms (loss + gradient, one call) at RPN scale, N = %d; us per call, median (min, max) of %d groups' % (RPN_N, args.iters))
    g = torch.Generator(device=DEV).manual_seed(1)
    N = RPN_N
    p, t = torch.randn((N, 4), generator=g, device=DEV), torch.randn((N, 4), generator=g, device=DEV)
    w = (torch.rand((N, 4), generator=g, device=DEV) < 0.1).float()
    for rule, fn in (('smooth_l1', smooth_l1_c), ('balanced_l1', balanced_l1_c), ('mse', mse_c)):
        prm = dict(beta=1.0 / 9.0) if rule == 'smooth_l1' else {}
        res = timed([lambda i: native.reg_loss(rule, p, t, w, avg=256.0, **prm), composite(fn, p, t, w, 256.0), copy_of(4 * N * 4 * 4)], args.iters, args.group)
        line_of(rule, '%d x 4' % N, res, lines, js)
    xy, wh = torch.rand((N, 2), generator=g, device=DEV) * 500, 8 + torch.rand((N, 2), generator=g, device=DEV) * 100
    bt = torch.cat([xy, xy + wh], 1)
    bp = bt + torch.randn((N, 4), generator=g, device=DEV) * 6
    w_row = (torch.rand(N, generator=g, device=DEV) < 0.1).float()
    res = timed([lambda i: native.box_loss('iou', bp, bt, w_row, eps=1e-6, avg=256.0), composite(iou_c, bp, bt, w_row, 256.0), copy_of(N * 4 * (12 + 1))],
                args.iters, args.group)
    line_of('iou', '%d pairs' % N, res, lines, js)
    res = timed([lambda i: native.box_loss('bounded_iou', bp, bt, w, avg=256.0), composite(bounded_iou_c, bp, bt, w, 256.0), copy_of(4 * N * 4 * 4)],
                args.iters, args.group)
    line_of('bounded_iou', '%d pairs' % N, res, lines, js)


def ghm_report(args, lines, js):
    lines.append('')
    lines.append('GHM (zero, histogram, finalize, loss + gradient, merge: five launches, no host read), bins 10, momentum 0; the composite is ghm_loss.py')
    lines.append('without its per-bin .item() loop (bucketize + bincount on the device), forward + backward')
    g = torch.Generator(device=DEV).manual_seed(2)
    for kind, N, C in (('ghmc', 150000, 80), ('ghmc', RPN_N, 1), ('ghmr', RPN_N, 4)):
        edges = torch.arange(11, device=DEV).float() / 10
        edges[-1] = edges[-1] + 1e-6 if kind == 'ghmc' else 1e3
        p = torch.randn((N, C), generator=g, device=DEV) * (2.5 if kind == 'ghmc' else 0.05)
        t = (torch.rand((N, C), generator=g, device=DEV) < 0.05).float() if kind == 'ghmc' else torch.zeros((N, C), device=DEV)
        w = (torch.rand((N, C), generator=g, device=DEV) < 0.8).float()
        comp = ghm_c(kind, edges)
        if kind == 'ghmc':
            call = lambda i: native.ghmc_loss(p, t, w, edges)      # noqa: E731
        else:
            call = lambda i: native.ghmr_loss(p, t, w, edges, 0.02)      # noqa: E731
        res = timed([call, lambda i: comp(p, t, w), copy_of(N * C * 4 * 7)], args.iters, args.group)     # two passes over three inputs, one output
        line_of(kind, '%d x %d' % (N, C), res, lines, js)


def train_report(args, lines, js):
    T, HW, PAD = 3, (600, 1000), (608, 1008)
    imgs = torch.cat([S.synth_frame(300 + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    gt_b = torch.tensor([[100., 120., 420., 380.], [500., 200., 830., 560.], [300., 60., 380., 200.]]).to(DEV)
    gt_l = torch.tensor([5, 12, 30]).to(DEV)
    models = {}
    for which in ('SmoothL1Loss', 'BalancedL1Loss'):
        cfg = selsa_train_config(ohem=False)
        cfg.model.rpn_head['loss_bbox'] = dict(type=which, beta=1.0 / 9.0, loss_weight=1.0)
        cfg.model.bbox_head['loss_bbox'] = dict(type=which, beta=1.0, loss_weight=1.0)
        models[which] = hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, S.synth_state_dict('selsa'), torch.float32, DEV))

    def step(model):
        for p in model.parameters():
            p.grad = None
        out = model(imgs, metas, return_loss=True, gt_bboxes=[gt_b] * T, gt_labels=[gt_l] * T)
        sum((v if isinstance(v, torch.Tensor) else sum(v)).sum() for k, v in out.items() if 'loss' in k).backward()
        return out

    lines.append('')
    lines.append('one SELSA training iteration (T = %d, %d x %d, f32, forward + backward, no OHEM), ms per iteration (median of %d), the two configs alternating %d times:'
                 % (T, PAD[0], PAD[1], args.steps, args.reps))
    for rep in range(args.reps):
        row = []
        for which, model in models.items():
            for _ in range(2):
                out = step(model)
            ms = []
            for _ in range(args.steps):
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = step(model)
                e.record()
                torch.cuda.synchronize()
                ms.append(s.elapsed_time(e))
            row.append('%s %.2f (min %.2f, max %.2f; loss_bbox %.4g)' % (which, statistics.median(ms), min(ms), max(ms), float(out['loss_bbox'])))
            js.setdefault('train %s ms' % which, []).append(statistics.median(ms))
        lines.append('  round %d: ' % (rep + 1) + '   '.join(row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--group', type=int, default=40, help='launches between two events (fewer for calls slower than 0.125 ms: a group is 5 ms at most)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--only', choices=['reduced', 'ghm', 'train'], default=None, help='one section (a caller that gives every section a time limit of its own)')
    ap.add_argument('--out', default=None, help='the report as a file; with --only the section is appended')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('loss_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    if args.only in (None, 'reduced'):
        lines.append('tools/loss_bench.py on %s' % torch.cuda.get_device_name(0))
        reduced_report(args, lines, js)
    if args.only in (None, 'ghm'):
        ghm_report(args, lines, js)
    if args.only == 'train' or (args.only is None and not args.no_train):
        train_report(args, lines, js)
    if args.out:
        with open(args.out, 'a' if args.only else 'w') as f:
            f.write('\n'.join(lines) + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
