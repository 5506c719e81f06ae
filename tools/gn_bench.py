"""Cost of the group-norm kernels (csrc/gn.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then the median of
--iters groups of back-to-back launches; the calls that are compared at one shape take turns group by group, so that a drift of the
clocks or a neighbour on the host meets all of them alike -- tools/gconv_bench.py's method):

  steps     native.group_norm_stats and native.group_norm_apply (plain, with a residual, with a normalised residual; ReLU on) on 15
            frames of 152 x 252 x 256 (layer 1), 76 x 126 x 512 (layer 2) and 38 x 63 x 1024 (layer 3), 32 groups, in bf16 / f16 /
            f32, beside the project's own copy of the same map, native.avgpool_nhwc(x, 1).  Every call walks a ring of maps larger
            than the 256 MB last-level cache.  Bytes are derived from the shapes (stats: the map once; copy: the map twice; apply:
            two maps, three with a residual), no counter was read.  The yardstick: stats time <= copy time, apply-with-residual
            time <= 1.5 x copy time; both ratios are printed, from medians, with YES / NO per shape and mode.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) of R-50 under GroupNorm against the
            R-50 with frozen BatchNorm, and against that R-50 with its fused closes and its dead-pixel skip switched off (every
            stage at full resolution, one launch per conv: what the GroupNorm net's convs cost without their norms), the three
            alternating --reps times.  --no-window skips it.

    python tools/gn_bench.py [--iters 30] [--out profiles/gn_bench.txt]

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
from hvrnet_amd import backbone, native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tools.gconv_bench import DEV, FRAMES, LLC_BYTES, Report, timed  # noqa: E402

MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
SHAPES = [('layer1', 152, 252, 256), ('layer2', 76, 126, 512), ('layer3', 38, 63, 1024)]
G = 32
GN = dict(type='GN', num_groups=G)


def steps_report(args, lines, js):
    lines.append('stats / apply of a GroupNorm(%d, C) on %d frames; us per call, median (min, max) of %d groups;' % (G, FRAMES, args.iters))
    lines.append('bytes derived from the shapes: stats = the map once, copy = the map twice, apply = two maps (u, y), with a residual three')
    for name, H, W, C in SHAPES:
        g = torch.Generator().manual_seed(3)
        ga, be, gr, br = [(t.to(DEV)) for t in (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5,
                                                 torch.randn(C, generator=g) * 0.1)]
        for mname, dt in MODES:
            gen = torch.Generator(device=DEV).manual_seed(1)
            x = torch.randn((FRAMES, H, W, C), generator=gen, device=DEV).to(dt)
            nbytes = x.numel() * x.element_size()
            n = max(2, min(8, int(2 * LLC_BYTES // nbytes) + 1))
            xs = [x] + [x.clone() for _ in range(n - 1)]
            ys = [torch.empty_like(x) for _ in range(n)]
            ident = [x.clone() for _ in range(n)]
            ws = native.group_norm_stats(x, G)
            wr = native.group_norm_stats(ident[0], G)
            calls = [lambda i: native.group_norm_stats(xs[i % n], G),
                     lambda i: native.avgpool_nhwc(xs[i % n], 1, out=ys[i % n]),
                     lambda i: native.group_norm_apply(xs[i % n], ws, ga, be, 1e-5, G, relu=True, out=ys[i % n]),
                     lambda i: native.group_norm_apply(xs[i % n], ws, ga, be, 1e-5, G, ident[i % n], None, True, out=ys[i % n]),
                     lambda i: native.group_norm_apply(xs[i % n], ws, ga, be, 1e-5, G, ident[i % n], (wr, gr, br), True, out=ys[i % n])]
            ts, tc, tp, tr, tn = timed(calls, args.iters, args.group)
            head = '  %-7s %3dx%-3d C %4d %-4s' % (name, H, W, C, mname)
            lines.append('%s  stats %7.1f us (%.1f, %.1f) %5.2f TB/s   copy %7.1f us (%.1f, %.1f) %5.2f TB/s   apply %7.1f us (%.1f, %.1f) %5.2f TB/s   '
                         'apply + resid %7.1f us (%.1f, %.1f) %5.2f TB/s   apply + normalised resid %7.1f us (%.1f, %.1f)   S = %d'
                         % (head, ts[0], ts[1], ts[2], nbytes / ts[0] / 1e6, tc[0], tc[1], tc[2], 2 * nbytes / tc[0] / 1e6, tp[0], tp[1], tp[2],
                            2 * nbytes / tp[0] / 1e6, tr[0], tr[1], tr[2], 3 * nbytes / tr[0] / 1e6, tn[0], tn[1], tn[2],
                            native.group_norm_splits(FRAMES, H * W, C)))
            ok_s, ok_a = ts[0] <= tc[0], tr[0] <= 1.5 * tc[0]
            lines.append('%s  stats / copy = %.2f (expected <= 1: %s)   apply + resid / copy = %.2f (expected <= 1.5: %s)   a whole norm (stats + apply) %.1f us'
                         % (' ' * len(head), ts[0] / tc[0], 'YES' if ok_s else 'NO', tr[0] / tc[0], 'YES' if ok_a else 'NO', ts[0] + tp[0]))
            js['%s %s' % (name, mname)] = dict(stats_us=ts[0], copy_us=tc[0], apply_us=tp[0], apply_resid_us=tr[0], apply_normed_us=tn[0],
                                               stats_over_copy=ts[0] / tc[0], apply_resid_over_copy=tr[0] / tc[0], stats_ok=ok_s, apply_ok=ok_a)
            del xs, ys, ident
            torch.cuda.empty_cache()


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which in ('R-50', 'R-50 unfused, full resolution', 'R-50-GN'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        cfg.model.backbone = dict(cfg.model.backbone, depth=50)
        cfg.model.shared_head = dict(cfg.model.shared_head, depth=50)
        sd = S.synth_state_dict('hvr', depth=50)
        if 'GN' in which:
            cfg.model.backbone = dict(cfg.model.backbone, norm_cfg=GN)
            cfg.model.shared_head = dict(cfg.model.shared_head, norm_cfg=GN)
            sd = S.synth_state_dict('hvr', depth=50, norm='GN')
        model = hvrnet_amd.build_model(cfg, sd, torch.bfloat16, DEV)
        knobs = (backbone.Bottleneck.fuse_next, backbone.Bottleneck.fuse_tail, backbone.ResNet.skip_dead_pixels)
        if 'unfused' in which:   # (class attributes: the routes are planned while the graph is captured)
            backbone.Bottleneck.fuse_next = backbone.Bottleneck.fuse_tail = backbone.ResNet.skip_dead_pixels = False
        try:
            graphs[which] = GraphedClip(model, clip, metas, rescale=True)
        finally:
            backbone.Bottleneck.fuse_next, backbone.Bottleneck.fuse_tail, backbone.ResNet.skip_dead_pixels = knobs
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the three models alternating %d times (R-50-GN: 53 norms = 49 stats + apply pairs and 4 shortcut stats passes; no fused stem):' % args.reps)
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
    bn, un, gn = [statistics.median(js['window %s ms' % k]) for k in graphs]
    lines.append('  medians: R-50 %.2f ms, unfused at full resolution %.2f ms, R-50-GN %.2f ms: of the gap of %.2f ms, %.2f ms (%.0f%%) is what the fused closes and '
                 'the dead-pixel skip save a BatchNorm net,' % (bn, un, gn, gn - bn, un - bn, 100.0 * (un - bn) / max(gn - bn, 1e-9)))
    lines.append('  the remaining %.2f ms the 53 norms (and the unfused stem): %.1f us per norm' % (gn - un, 1e3 * (gn - un) / 53))
    js['per norm us'] = 1e3 * (gn - un) / 53


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
        sys.exit('gn_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/gn_bench.py on %s' % torch.cuda.get_device_name(0))
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
