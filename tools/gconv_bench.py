"""Cost of the grouped 3x3 conv (csrc/gconv3x3.hip, native.conv3x3_grouped) on an otherwise idle MI355X, in one process, HIP-event
times (warm-up, then the median of --iters groups of back-to-back launches; slow calls get shorter groups; the calls that are compared
at one shape -- automatic route, route='dense', the ResNet's conv -- take turns group by group, so that a drift of the clocks or a
neighbour on the host meets all of them alike):

  kernel    conv2 of ResNeXt-101 32x4d at the stage shapes of a 15-frame 608 x 1008 window -- 152 x 252 x 128 at Cg 4, 76 x 126 x 256 at
            Cg 8, 38 x 63 x 512 at Cg 16, 38 x 63 x 1024 at Cg 32 with dilation 2, and the stride-2 first blocks of layers 2 and 3 -- in
            every compute mode: the route the automatic choice takes, the same call with route='dense' (conv2d_nhwc on the block-diagonal
            weight), and ResNet-101's plain 3x3 of that stage (half the channels).  Every call cycles through a ring of input / output
            buffers larger than the 256 MB last-level cache, so a time is not that of a map that stayed on the chip.  Beside each time
            the bytes the rule must move (map in + map out + weights, computed from the shape) and the rate that gives against the
            8 TB/s HBM peak (MI355X_MICROARCH): a derived figure, no counter was read.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) with ResNeXt-101 32x4d + ResXLayer
            (pytorch style, as the published ResNeXt checkpoints are) against ResNet-101 + ResLayer (the benchmark's caffe-style model),
            alternating --reps times.  --no-window skips it.

    python tools/gconv_bench.py [--iters 30] [--out profiles/gconv_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.  The last line of the kernel section says
whether the automatic route beat route='dense' at every shape where it picked the grouped kernel.
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

DEV = 'cuda:0'
HBM_PEAK = 8.0e12
LLC_BYTES = 256e6
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f16x2', native.SPLIT), ('f32', torch.float32)]
FRAMES = 15
# name, H, W of the input map, C, Cg, stride, dilation
SHAPES = [('layer1', 152, 252, 128, 4, 1, 1), ('layer2.0 /2', 152, 252, 256, 8, 2, 1), ('layer2', 76, 126, 256, 8, 1, 1),
          ('layer3.0 /2', 76, 126, 512, 16, 2, 1), ('layer3', 38, 63, 512, 16, 1, 1), ('res5 d2', 38, 63, 1024, 32, 1, 2)]


class Report(list):
    """The report's lines, printed as they come (a run that ends early leaves what it measured)."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def timed(fns, iters, group, warmup=2):
    """-> [(median, min, max) microseconds of one call of fn(i)] for the fns, which take turns: per round, `group` calls of each between
    two events (fewer when a call is slow: a group is about 5 ms of work at most, a figure the median of `iters` such groups)."""
    n, groups = 0, []
    for fn in fns:
        for _ in range(warmup):
            fn(n)
            n += 1
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(n)
        e.record()
        torch.cuda.synchronize()
        groups.append(max(1, min(group, int(5000.0 / max(s.elapsed_time(e) * 1e3, 1.0)))))
    us = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(groups[k]):
                n += 1
                fn(n)
            e.record()
            torch.cuda.synchronize()
            us[k].append(s.elapsed_time(e) * 1e3 / groups[k])
    return [(statistics.median(u), min(u), max(u)) for u in us]


def operand(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(shape, generator=g, device=DEV).clamp(min=0.0)
    return native.cast(t, native.SPLIT) if dtype == native.SPLIT else t.to(dtype)


def ring_of(x, out_shape, nbytes):
    """Copies of x and output buffers, enough of them that one pass over the ring moves more than twice the last-level cache."""
    n = max(2, min(8, int(2 * LLC_BYTES // max(nbytes, 1)) + 1))
    return [x] + [x.clone() for _ in range(n - 1)], [torch.empty(out_shape, dtype=x.dtype, device=DEV) for _ in range(n)]


def kernel_report(args, lines, js):
    lines.append('grouped 3x3 + bias + ReLU at the stage shapes of X-101 32x4d, %d frames; us per call, median (min, max);' % FRAMES)
    lines.append('bytes = map in + map out + weights of the grouped rule (derived from the shape), rate = bytes / time against the 8 TB/s HBM peak (derived)')
    verdict = []
    for name, H, W, C, Cg, s, d in SHAPES:
        OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
        for mname, dt in MODES:
            g = torch.Generator().manual_seed(7)
            w32 = (torch.randn((C, 3, 3, Cg), generator=g) / (9 * Cg) ** 0.5).to(DEV)
            gw = native.GroupedWeight(w32, dt)
            bias = torch.zeros(C, device=DEV)
            x = operand((FRAMES, H, W, C), dt, 1)
            es = x.element_size()
            nbytes = (FRAMES * H * W * C + FRAMES * OH * OW * C + 9 * C * Cg) * es
            xs, ys = ring_of(x, (FRAMES, OH, OW, C), (FRAMES * H * W * C + FRAMES * OH * OW * C) * es)
            n = len(xs)
            auto = 'grouped' if native.conv3x3_grouped_supported(FRAMES, H, W, C, C // Cg, s, d, dt) else 'dense'
            # ResNet-101's conv2 of the same stage: half the channels, dense
            P = C // 2
            xp = operand((FRAMES, H, W, P), dt, 2)
            wp = native.as_operand((torch.randn((P, 3, 3, P), generator=g) / (9 * P) ** 0.5).to(DEV), dt)
            bp = torch.zeros(P, device=DEV)
            xps, yps = ring_of(xp, (FRAMES, OH, OW, P), (FRAMES * H * W * P + FRAMES * OH * OW * P) * es)
            m = len(xps)
            fns = [lambda i: native.conv3x3_grouped(xs[i % n], gw, bias, True, s, d, out=ys[i % n]),
                   lambda i: native.conv2d_nhwc(xps[i % m], wp, bp, relu=True, stride=s, pad=d, dil=d, out=yps[i % m])]
            if auto == 'grouped':
                fns.append(lambda i: native.conv3x3_grouped(xs[i % n], gw, bias, True, s, d, out=ys[i % n], route='dense'))
            res = timed(fns, args.iters, args.group)
            ta, tp, td = res[0], res[1], res[-1] if auto == 'grouped' else res[0]
            lines.append('  %-12s %3dx%-3d C %4d Cg %2d s%d d%d %-5s  auto = %-7s %8.1f us (%.1f, %.1f)  %6.1f MB -> %5.2f TB/s (%4.1f %% of peak)   route=dense %9.1f us (%.1f, %.1f)   R-101 plain 3x3 (%d ch) %8.1f us'
                         % (name, H, W, C, Cg, s, d, mname, auto, ta[0], ta[1], ta[2], nbytes / 1e6, nbytes / ta[0] / 1e6, 100 * nbytes / ta[0] * 1e6 / HBM_PEAK,
                            td[0], td[1], td[2], P, tp[0]))
            key = '%s %s' % (name, mname)
            js[key + ' auto'] = auto
            js[key + ' auto us'] = ta[0]
            js[key + ' dense us'] = td[0]
            js[key + ' r101 us'] = tp[0]
            if auto == 'grouped':
                verdict.append((key, ta[0] < td[0]))
            del x, xs, ys, xp, xps, yps, gw
            torch.cuda.empty_cache()
    slower = [k for k, ok in verdict if not ok]
    lines.append('automatic route = grouped kernel at %d (shape, mode) pairs; faster than route=\'dense\' in this run at %d of them%s'
                 % (len(verdict), len(verdict) - len(slower), '' if not slower else ' -- NOT at: ' + ', '.join(slower)))
    js['grouped faster than dense everywhere it is chosen'] = not slower


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which in ('R-101 + ResLayer', 'X-101 32x4d + ResXLayer'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        sd = S.synth_state_dict('hvr')
        if which.startswith('X'):
            cfg.model.backbone = dict(type='ResNeXt', depth=101, groups=32, base_width=4, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1),
                                      out_indices=(2,), frozen_stages=1, style='pytorch', norm_eval=True)
            cfg.model.shared_head = dict(type='ResXLayer', depth=101, stage=3, stride=1, dilation=2, groups=32, base_width=4, style='pytorch',
                                         norm_eval=True, external_conv=True)
            sd = S.synth_state_dict('hvr', groups=32, base_width=4)
        model = hvrnet_amd.build_model(cfg, sd, torch.bfloat16, DEV)
        graphs[which] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the two models alternating %d times:' % args.reps)
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
        sys.exit('gconv_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/gconv_bench.py on %s' % torch.cuda.get_device_name(0))
    kernel_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
