"""Cost of the sigmoid focal loss kernels (csrc/focal.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then
the median of --iters groups of back-to-back launches; the calls compared at one shape take turns group by group -- tools/gconv_bench.py's
method):

  steps   native.sigmoid_focal_loss_fwd / _bwd and the reduced form native.focal_loss at N x C = 2394 x 12 and 150000 x 80, f32 and bf16
          logits (the reduced form reads f32 only).  Bytes are derived from the shapes -- forward: the logits once and the f32 loss once;
          backward: the logits, d_loss and d_logits; reduced: the f32 logits once and d_logits once -- and printed as achieved bytes/s
          beside the 8 TB/s HBM peak the README uses.  No counter was read.  The large shape walks a ring of inputs larger than the
          256 MB last-level cache.
  rpn     native.rpn_focal_loss beside native.rpn_loss on 38 x 63 positions of 12 anchors (ld = 64).
  train   one SELSA training iteration (forward + backward, T = 3, 608 x 1008, the built-in training config) with the focal RPN
          (loss_cls = FocalLoss) beside the same model through the CrossEntropyLoss config, alternating --reps times.  --no-train
          skips it.

    python tools/focal_bench.py [--iters 30] [--out profiles/focal_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, synthetic as S  # noqa: E402
from hvrnet_amd.config import selsa_train_config  # noqa: E402
from tools.gconv_bench import DEV, HBM_PEAK, LLC_BYTES, Report, timed  # noqa: E402

SHAPES = [(2394, 12), (150000, 80)]
MODES = [('f32', torch.float32), ('bf16', torch.bfloat16)]


def steps_report(args, lines, js):
    lines.append('elementwise forward / backward and the reduced form, gamma 2, alpha 0.25; us per call, median (min, max) of %d groups;' % args.iters)
    lines.append('bytes derived from the shapes; HBM peak %.0f TB/s' % (HBM_PEAK / 1e12))
    for N, C in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(1)
        t = torch.randint(-1, C + 1, (N,), generator=g, device=DEV)
        w = torch.rand(N, generator=g, device=DEV) + 0.5
        for mname, dt in MODES:
            x = (torch.randn((N, C), generator=g, device=DEV) * 4.0).to(dt)
            nin, nout = x.numel() * x.element_size(), N * C * 4
            n = max(2, min(8, int(2 * LLC_BYTES // (nin + 2 * nout)) + 1))
            xs = [x] + [x.clone() for _ in range(n - 1)]
            ds = [torch.rand((N, C), generator=g, device=DEV) for _ in range(n)]
            calls = [lambda i: native.sigmoid_focal_loss_fwd(xs[i % n], t, 2.0, 0.25),
                     lambda i: native.sigmoid_focal_loss_bwd(xs[i % n], t, ds[i % n], 2.0, 0.25)]
            if dt == torch.float32:
                calls.append(lambda i: native.focal_loss(xs[i % n], t, w, 2.0, 0.25, 1.0, float(N * C)))
            res = timed(calls, args.iters, args.group)
            tf, tb = res[0], res[1]
            line = ('  %6d x %-2d %-4s  forward %8.1f us (%.1f, %.1f) %5.2f TB/s   backward %8.1f us (%.1f, %.1f) %5.2f TB/s'
                    % (N, C, mname, tf[0], tf[1], tf[2], (nin + nout) / tf[0] / 1e6, tb[0], tb[1], tb[2], (nin + 2 * nout) / tb[0] / 1e6))
            js['%dx%d %s' % (N, C, mname)] = dict(fwd_us=tf[0], bwd_us=tb[0], fwd_TBps=(nin + nout) / tf[0] / 1e6, bwd_TBps=(nin + 2 * nout) / tb[0] / 1e6)
            if dt == torch.float32:
                tr = res[2]
                line += ('   reduced (loss + gradient, two launches) %8.1f us (%.1f, %.1f) %5.2f TB/s = %.0f%% of the HBM peak, S = %d'
                         % (tr[0], tr[1], tr[2], (nin + nout) / tr[0] / 1e6, 100.0 * (nin + nout) / tr[0] / 1e6 / (HBM_PEAK / 1e12),
                            native.focal_loss_splits(N, C)))
                js['%dx%d %s' % (N, C, mname)].update(reduced_us=tr[0], reduced_TBps=(nin + nout) / tr[0] / 1e6)
            lines.append(line)
            del xs, ds
            torch.cuda.empty_cache()


def rpn_report(args, lines, js):
    H, W, A, ld = 38, 63, 12, 64
    rows, M = H * W, H * W * A
    g = torch.Generator(device=DEV).manual_seed(2)
    o = torch.randn((rows, ld), generator=g, device=DEV) * 3.0
    labels = (torch.rand(M, generator=g, device=DEV) < 0.01).long()
    lw = (torch.rand(M, generator=g, device=DEV) < 0.5).float()
    bt = torch.randn((M, 4), generator=g, device=DEV)
    bw = labels.float()[:, None].expand(-1, 4).contiguous()
    counts = torch.tensor([int(labels.sum()), int(((labels == 0) & (lw > 0)).sum())], dtype=torch.int32, device=DEV)
    tf, tb = timed([lambda i: native.rpn_focal_loss(o, A, labels, lw, bt, bw, counts, 1.0 / 9.0, 2.0, 0.25),
                    lambda i: native.rpn_loss(o, A, labels, lw, bt, bw, counts, 1.0 / 9.0)], args.iters, args.group)
    lines.append('')
    lines.append('RPN loss on %d x %d positions of %d anchors (ld = %d), one workgroup each: hvr_rpn_focal_loss %.1f us (%.1f, %.1f)   hvr_rpn_loss %.1f us (%.1f, %.1f)'
                 % (H, W, A, ld, tf[0], tf[1], tf[2], tb[0], tb[1], tb[2]))
    js['rpn'] = dict(focal_us=tf[0], bce_us=tb[0])


def train_report(args, lines, js):
    T, HW, PAD = 3, (600, 1000), (608, 1008)
    imgs = torch.cat([S.synth_frame(300 + i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    gt_b = torch.tensor([[100., 120., 420., 380.], [500., 200., 830., 560.], [300., 60., 380., 200.]]).to(DEV)
    gt_l = torch.tensor([5, 12, 30]).to(DEV)
    models = {}
    for which in ('BCE RPN (CrossEntropyLoss, 256 sampled anchors)', 'focal RPN (FocalLoss, every assigned anchor)'):
        cfg = selsa_train_config()
        if which.startswith('focal'):
            cfg.model.rpn_head['loss_cls'] = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
        models[which] = hvrnet_amd.enable_training(hvrnet_amd.build_model(cfg, S.synth_state_dict('selsa'), torch.float32, DEV))

    def step(model):
        for p in model.parameters():
            p.grad = None
        out = model(imgs, metas, return_loss=True, gt_bboxes=[gt_b] * T, gt_labels=[gt_l] * T)
        sum((v if isinstance(v, torch.Tensor) else sum(v)).sum() for k, v in out.items() if 'loss' in k).backward()
        return out

    lines.append('')
    lines.append('one SELSA training iteration (T = %d, %d x %d, f32, forward + backward), ms per iteration (median of %d), the two configs alternating %d times:'
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
            row.append('%s %.2f (min %.2f, max %.2f; loss_rpn_cls %.4g)' % (which, statistics.median(ms), min(ms), max(ms), float(out['loss_rpn_cls'][0])))
            js.setdefault('train %s ms' % which.split(' (')[0], []).append(statistics.median(ms))
        lines.append('  round %d: ' % (rep + 1) + '   '.join(row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--group', type=int, default=40, help='launches between two events (fewer for calls slower than 0.125 ms: a group is 5 ms at most)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--only', choices=['steps', 'rpn', 'train'], default=None, help='one section (a caller that gives every section a time limit of its own)')
    ap.add_argument('--out', default=None, help='the report as a file; with --only the section is appended')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('focal_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    if args.only in (None, 'steps'):
        lines.append('tools/focal_bench.py on %s' % torch.cuda.get_device_name(0))
        steps_report(args, lines, js)
    if args.only in (None, 'rpn'):
        rpn_report(args, lines, js)
    if args.only == 'train' or (args.only is None and not args.no_train):
        train_report(args, lines, js)
    if args.out:
        with open(args.out, 'a' if args.only else 'w') as f:
            f.write('\n'.join(lines) + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
