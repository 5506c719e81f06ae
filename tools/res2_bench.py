"""Cost of the Res2Net kernels (csrc/res2.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then the median of
--iters groups of back-to-back launches; slow calls get shorter groups; the calls that are compared at one shape take turns group by
group, so that a drift of the clocks or a neighbour on the host meets all of them alike -- tools/gconv_bench.py's method):

  branch    one branch conv of a Bottle2neck (native.res2_conv3x3: slice 1 of the 4 Wp-channel map P, slice 0 of Q added where the block
            is a 'normal' one, into slice 1 of Q) at the four stage shapes of a 15-frame 608 x 1008 window -- 152 x 252 at Wp 32,
            76 x 126 at Wp 64, 38 x 63 at Wp 128, 38 x 63 at Wp 224 with dilation 2 -- and the stride-2 'stage' blocks of layers 2 and
            3, in bf16 and half: route='kernel' against route='composite' (slice copy, torch add and rounding, conv2d_nhwc, copy back:
            calls older than the kernel), and which of the two the automatic route takes.  f32 and split half have the composite
            route only; it is timed alone.  Every call cycles through a ring of P / Q maps larger than the 256 MB last-level cache.
            Beside each time the flops of the rule with the real width (2 x 9 x width^2 per output pixel) and the bytes it must move
            (slice in, added slice in, slice out, weights; derived from the shape, no counter was read).  A kernel counts as faster
            only where its slowest group is faster than the composite route's fastest.
  pool      native.avgpool_nhwc in its three uses at the layer-2 shapes (bf16), native.stem3x3s2_first and the whole deep stem beside
            ResNet's fused 7x7 stem on 15 frames.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) with Res2Net-101 + Res2Layer against
            ResNet-101 + ResLayer (the benchmark's caffe-style model), alternating --reps times.  --no-window skips it.

    python tools/res2_bench.py [--iters 30] [--out profiles/res2_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.  The last line of the branch section says
whether the kernel beat the composite route at every (shape, mode) pair where the automatic route picks it.
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
from tools.gconv_bench import DEV, FRAMES, LLC_BYTES, Report, operand, timed  # noqa: E402

KERNEL_MODES = [('bf16', torch.bfloat16), ('f16', torch.float16)]
OTHER_MODES = [('f16x2', native.SPLIT), ('f32', torch.float32)]
# name, H, W of the input map, width, stride, dilation, with the pre-add
SHAPES = [('layer1', 152, 252, 26, 1, 1, True), ('layer2.0 /2', 152, 252, 52, 2, 1, False), ('layer2', 76, 126, 52, 1, 1, True),
          ('layer3.0 /2', 76, 126, 104, 2, 1, False), ('layer3', 38, 63, 104, 1, 1, True), ('res5.0 d1', 38, 63, 208, 1, 1, False),
          ('res5 d2', 38, 63, 208, 1, 2, True)]


def rings(H, W, OH, OW, Wp, dt, with_add):
    """P / Q maps of 4 Wp channels, enough of them that one pass over the ring moves more than twice the last-level cache."""
    es = 4 if dt in (native.SPLIT, torch.float32) else 2
    moved = (FRAMES * H * W * Wp * (2 if with_add else 1) + FRAMES * OH * OW * Wp) * es
    n = max(2, min(8, int(2 * LLC_BYTES // max(moved, 1)) + 1))
    P = operand((FRAMES, H, W, 4 * Wp), dt, 1)
    Q = operand((FRAMES, OH, OW, 4 * Wp), dt, 2)
    return [P] + [P.clone() for _ in range(n - 1)], [Q] + [Q.clone() for _ in range(n - 1)], moved


def branch_report(args, lines, js):
    lines.append('one branch conv of a Bottle2neck (3x3 over a Wp-channel slice + bias + ReLU, with the pre-add where marked), %d frames;' % FRAMES)
    lines.append('us per call, median (min, max) of %d groups; flops = 2 x 9 x width^2 per output pixel, bytes = slices in + slice out + weights (derived)' % args.iters)
    verdict = []
    for name, H, W, width, s, d, with_add in SHAPES:
        Wp = native.res2_pad_width(width)
        OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
        flops = 2.0 * 9 * width * width * FRAMES * OH * OW
        g = torch.Generator().manual_seed(7)
        w32 = torch.zeros((Wp, 3, 3, Wp))
        w32[:width, :, :, :width] = torch.randn((width, 3, 3, width), generator=g) / (9 * width) ** 0.5
        bias = torch.zeros(Wp, device=DEV)
        for mname, dt in KERNEL_MODES + OTHER_MODES:
            rw = native.Res2Weight(w32.to(DEV), dt)
            Ps, Qs, moved = rings(H, W, OH, OW, Wp, dt, with_add)
            n = len(Ps)
            nbytes = moved + 9 * Wp * Wp * Ps[0].element_size()

            def call(route):
                return lambda i: native.res2_conv3x3(Ps[i % n], Wp, rw, bias, add=Qs[i % n] if with_add else None, add_off=0, out=Qs[i % n], out_off=Wp,
                                                     stride=s, dil=d, relu=True, route=route)
            key = '%s %s' % (name, mname)
            head = '  %-12s %3dx%-3d width %3d Wp %3d s%d d%d %s %-5s' % (name, H, W, width, Wp, s, d, '+add' if with_add else '    ', mname)
            if dt in (torch.bfloat16, torch.float16):
                auto = 'kernel' if Wp in native.RES2_KERNEL_WIDTHS.get(dt, ()) and native.res2_conv3x3_supported(FRAMES, H, W, Wp, s, d, dt) else 'composite'
                tk, tc = timed([call('kernel'), call('composite')], args.iters, args.group)
                lines.append('%s  kernel %8.1f us (%.1f, %.1f)  %6.1f TF/s  %6.1f MB -> %5.2f TB/s   composite %8.1f us (%.1f, %.1f)   auto = %s'
                             % (head, tk[0], tk[1], tk[2], flops / tk[0] / 1e6, nbytes / 1e6, nbytes / tk[0] / 1e6, tc[0], tc[1], tc[2], auto))
                js[key + ' kernel us'], js[key + ' composite us'], js[key + ' auto'] = tk[0], tc[0], auto
                if auto == 'kernel':
                    verdict.append((key, tk[2] < tc[1]))
            else:
                tc, = timed([call('composite')], args.iters, args.group)
                lines.append('%s  composite %8.1f us (%.1f, %.1f)  (the only route of this mode)' % (head, tc[0], tc[1], tc[2]))
                js[key + ' composite us'] = tc[0]
            del Ps, Qs, rw
            torch.cuda.empty_cache()
    slower = [k for k, ok in verdict if not ok]
    lines.append('automatic route = slice kernel at %d (shape, mode) pairs; its slowest group faster than the composite route\'s fastest at %d of them%s'
                 % (len(verdict), len(verdict) - len(slower), '' if not slower else ' -- NOT at: ' + ', '.join(slower)))
    js['kernel faster than composite everywhere it is chosen'] = not slower


def pool_and_stem_report(args, lines, js):
    lines.append('')
    lines.append('average pool (bf16, %d frames) and the stems; us per call, median (min, max)' % FRAMES)
    dt = torch.bfloat16
    P = operand((FRAMES, 76, 126, 256), dt, 3)
    X = operand((FRAMES, 152, 252, 256), dt, 4)
    Q = torch.empty((FRAMES, 76, 126, 256), dtype=dt, device=DEV)
    cases = [('carried slice, copy (k 1), 76x126 x 64 of 256', lambda i: native.avgpool_nhwc(P, 1, 1, 0, False, True, x_off=192, C=64, out=Q, out_off=192)),
             ('\'stage\' pool (k 3 / 1, pad 1), 76x126 x 64 of 256', lambda i: native.avgpool_nhwc(P, 3, 1, 1, False, True, x_off=192, C=64, out=Q, out_off=192)),
             ('\'stage\' pool (k 3 / 2, pad 1), 152x252 x 64 of 256', lambda i: native.avgpool_nhwc(X, 3, 2, 1, False, True, x_off=192, C=64, out=Q, out_off=192)),
             ('shortcut pool (k 2 / 2, ceil), 152x252 x 256', lambda i: native.avgpool_nhwc(X, 2, 2, 0, True, False, out=Q))]
    for (what, _), t in zip(cases, timed([c[1] for c in cases], args.iters, args.group)):
        lines.append('  %-52s %8.1f us (%.1f, %.1f)' % (what, t[0], t[1], t[2]))
        js['pool ' + what + ' us'] = t[0]
    img = torch.cat([S.synth_frame(i) for i in range(FRAMES)], 0).to(DEV)
    r2 = hvrnet_amd.Res2Net(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,)).to(DEV)
    r1 = hvrnet_amd.ResNet(depth=101, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), style='caffe').to(DEV)
    p2, p1 = r2.packed(torch.device(DEV)), r1.packed(torch.device(DEV))
    cases = [('stem3x3s2_first alone (3 -> 32 of 64 channels, 608x1008)', lambda i: native.stem3x3s2_first(img, p2['s0'][0], p2['s0'][1], dt, channels=64)),
             ('Res2Net deep stem: first conv + two 3x3 convs + max pool', lambda i: r2._stem(img, p2)),
             ('ResNet stem: fused 7x7 / 2 + max pool', lambda i: r1._stem(img, p1))]
    with torch.no_grad():
        for (what, _), t in zip(cases, timed([c[1] for c in cases], args.iters, args.group)):
            lines.append('  %-60s %8.1f us (%.1f, %.1f)' % (what, t[0], t[1], t[2]))
            js['stem ' + what + ' us'] = t[0]


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which in ('R-101 + ResLayer', 'Res2Net-101 + Res2Layer'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        sd = S.synth_state_dict('hvr')
        if which.startswith('Res2'):
            cfg.model.backbone = dict(type='Res2Net', num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), frozen_stages=1,
                                      style='pytorch', norm_eval=True)
            cfg.model.shared_head = dict(type='Res2Layer', depth=101, stage=3, stride=1, dilation=2, style='pytorch', norm_eval=True, external_conv=True)
            sd = S.synth_state_dict('hvr', arch='res2net')
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
        sys.exit('res2_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/res2_bench.py on %s' % torch.cuda.get_device_name(0))
    branch_report(args, lines, js)
    pool_and_stem_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
