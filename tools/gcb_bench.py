"""Cost of the global context block kernels (csrc/gcb.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then
the median of --iters groups of back-to-back launches; the calls that are compared at one shape take turns group by group, so that a
drift of the clocks or a neighbour on the host meets all of them alike -- tools/gconv_bench.py's method):

  steps     native.gcb_pool, native.gcb_transform and native.gcb_apply (with the residual and the ReLU, as a Bottleneck runs it) on 15
            frames of 76 x 126 x 512 (layer 2) and 38 x 63 x 1024 (layer 3), ratio 1/16, 'att', add + mul, in every mode (split half
            runs the f32 kernels on the f32 form: its figures are the f32 ones plus the casts, which are not timed here), beside the
            project's own copy of the same map, native.avgpool_nhwc(x, 1).  The pool and the copy read a ring of maps larger than
            the 256 MB last-level cache.  Bytes are derived from the shapes (pool: the map once; copy: the map twice; apply: three
            maps), no counter was read.  The yardstick: pool time <= copy time, apply time <= 1.5 x copy time; both ratios are
            printed, from medians, with the (min, max) of the groups beside them.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) of R-101 with context blocks in
            layers 2 and 3 (ratio 1/16, att, add + mul) against the plain R-101 (the benchmark's model), alternating --reps times.
            --no-window skips it.

    python tools/gcb_bench.py [--iters 30] [--out profiles/gcb_bench.txt]

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
from hvrnet_amd.config import hvr_config  # noqa: E402
from tools.gconv_bench import DEV, FRAMES, LLC_BYTES, Report, timed  # noqa: E402

MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
SHAPES = [('layer2', 76, 126, 512), ('layer3', 38, 63, 1024)]
GCB = dict(ratio=1. / 16., pooling_type='att', fusion_types=('channel_add', 'channel_mul'))


def branch(g, C, R):
    return tuple(t.to(DEV).contiguous() for t in (torch.randn((R, C), generator=g) / C ** 0.5, torch.randn(R, generator=g) * 0.1, torch.rand(R, generator=g) + 0.5,
                                                  torch.randn(R, generator=g) * 0.1, torch.randn((R, C), generator=g) / R ** 0.5, torch.randn(C, generator=g) * 0.1))


def steps_report(args, lines, js):
    lines.append('pool / transform / apply of a context block (ratio 1/16, att, add + mul) on %d frames; us per call, median (min, max) of %d groups;' % (FRAMES, args.iters))
    lines.append('bytes derived from the shapes: pool = the map once, copy = the map twice, apply = three maps (u, identity, y)')
    ok = True
    for name, H, W, C in SHAPES:
        R = int(C * GCB['ratio'])
        g = torch.Generator().manual_seed(3)
        wm = (torch.randn(C, generator=g) * 2.0 / C ** 0.5).to(DEV)
        mul, add = branch(g, C, R), branch(g, C, R)
        for mname, dt in MODES:
            gen = torch.Generator(device=DEV).manual_seed(1)
            x = torch.randn((FRAMES, H, W, C), generator=gen, device=DEV).to(dt)
            nbytes = x.numel() * x.element_size()
            n = max(2, min(8, int(2 * LLC_BYTES // nbytes) + 1))
            xs = [x] + [x.clone() for _ in range(n - 1)]
            ys = [torch.empty_like(x) for _ in range(n)]
            ident = [x.clone() for _ in range(n)]
            part = native.gcb_pool(x, wm)
            m, t = native.gcb_transform(part, H * W, mul, add)
            calls = [lambda i: native.gcb_pool(xs[i % n], wm), lambda i: native.gcb_pool(xs[i % n], None), lambda i: native.avgpool_nhwc(xs[i % n], 1, out=ys[i % n]),
                     lambda i: native.gcb_apply(xs[i % n], m, t, ident[i % n], True, out=ys[i % n]), lambda i: native.gcb_transform(part, H * W, mul, add)]
            tp, tv, tc, ta, tt = timed(calls, args.iters, args.group)
            head = '  %-7s %3dx%-3d C %4d R %3d %-4s' % (name, H, W, C, R, mname)
            lines.append('%s  pool att %7.1f us (%.1f, %.1f) %5.2f TB/s   pool avg %7.1f us (%.1f, %.1f)   copy %7.1f us (%.1f, %.1f) %5.2f TB/s   apply %7.1f us (%.1f, %.1f) %5.2f TB/s   '
                         'transform %6.1f us (%.1f, %.1f)   S = %d' % (head, tp[0], tp[1], tp[2], nbytes / tp[0] / 1e6, tv[0], tv[1], tv[2], tc[0], tc[1], tc[2],
                                                                        2 * nbytes / tc[0] / 1e6, ta[0], ta[1], ta[2], 3 * nbytes / ta[0] / 1e6, tt[0], tt[1], tt[2],
                                                                        native.gcb_splits(FRAMES, H * W, C)))
            lines.append('%s  pool / copy = %.2f (expected <= 1)   apply / copy = %.2f (expected <= 1.5)' % (' ' * len(head), tp[0] / tc[0], ta[0] / tc[0]))
            key = '%s %s' % (name, mname)
            js[key] = dict(pool_us=tp[0], pool_avg_us=tv[0], copy_us=tc[0], apply_us=ta[0], transform_us=tt[0], pool_over_copy=tp[0] / tc[0], apply_over_copy=ta[0] / tc[0])
            ok = ok and tp[0] <= tc[0] and ta[0] <= 1.5 * tc[0]
            del xs, ys, ident
            torch.cuda.empty_cache()
    lines.append('the whole block (native.context_block with the residual and the ReLU: pool + transform + apply; split half: cast to f32, the f32 kernels, cast back):')
    for name, H, W, C in SHAPES:
        R = int(C * GCB['ratio'])
        g = torch.Generator().manual_seed(3)
        pk = dict(wm=(torch.randn(C, generator=g) * 2.0 / C ** 0.5).to(DEV), mul=branch(g, C, R), add=branch(g, C, R))
        row = []
        for mname, dt in MODES + [('f16x2', native.SPLIT)]:
            gen = torch.Generator(device=DEV).manual_seed(1)
            x = native.cast(torch.randn((FRAMES, H, W, C), generator=gen, device=DEV), dt)
            ident, y = x.clone(), torch.empty_like(x)
            tb, = timed([lambda i: native.context_block(x, pk, ident, True, out=y)], args.iters, args.group)
            row.append('%s %.1f us (%.1f, %.1f)' % (mname, tb[0], tb[1], tb[2]))
            js['%s %s block us' % (name, mname)] = tb[0]
            del x, ident, y
        lines.append('  %-7s %3dx%-3d C %4d  ' % (name, H, W, C) + '   '.join(row))
    lines.append('both expectations met at every (shape, mode): %s' % ('yes' if ok else 'NO'))
    js['expectations met'] = ok


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which in ('R-101', 'R-101 + gcb in layers 2-3'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        sd = S.synth_state_dict('hvr')
        if 'gcb' in which:
            cfg.model.backbone = dict(cfg.model.backbone, gcb=GCB, stage_with_gcb=(False, True, True))
            sd = S.synth_state_dict('hvr', gcb=GCB)
        model = hvrnet_amd.build_model(cfg, sd, torch.bfloat16, DEV)
        graphs[which] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the two models alternating %d times (27 context blocks: 4 in layer 2, 23 in layer 3; their stages run at full resolution):' % args.reps)
    for rep in range(args.reps):
        row = []
        for which, g in graphs.items():
            ms = []
            for _ in range(2):
                g.run(clip).result()
            for _ in range(args.windows):
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                pend = g.run(clip)
                e.record()
                pend.result()
                torch.cuda.synchronize()
                ms.append(s.elapsed_time(e))
            row.append((which, statistics.median(ms), min(ms), max(ms)))
            js.setdefault('window %s ms' % which, []).append(statistics.median(ms))
        lines.append('  round %d: ' % (rep + 1) + '   '.join('%s %.2f (min %.2f, max %.2f)' % r for r in row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--group', type=int, default=40, help='launches between two events (fewer for calls slower than 0.125 ms: a group is 5 ms at most)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('gcb_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/gcb_bench.py on %s' % torch.cuda.get_device_name(0))
    steps_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
