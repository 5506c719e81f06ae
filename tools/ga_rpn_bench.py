"""Cost of the Guided Anchoring RPN kernels (csrc/ga_rpn.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up,
then the median of --iters groups of back-to-back launches; the calls that are compared at one shape take turns group by group, so
that a drift of the clocks or a neighbour on the host meets all of them alike -- tools/gconv_bench.py's method):

  heads      the masked heads (native.masked_conv2d_nhwc, 1 + 4 outputs over concatenated weights, 1x1) at kept fractions 1.0, 0.3 and
             0.05 on 15 frames of the 38 x 63 map with C = 1024, in bf16, f16 and f32, beside the dense heads (native.conv2d_nhwc with
             the 5 rows padded to 8, f32 output) on the same map.  The maps come from a ring larger than the 256 MB last-level cache.
             The two comparisons that matter are printed as ratios of medians with the (min, max) of the groups beside the times:
             masked at 1.0 / dense, and masked at 0.3 / masked at 1.0.  Bytes are derived from the shapes (the kept rows of x once).
  mask       native.ga_mask_offsets (the keep map and the 72 offset channels of 4 deformable groups) on the same 15 frames.
  proposals  native.ga_rpn_proposals (kept fraction 0.5, nms_pre 2000, nms_post 300, max_num 300, nms_thr 0.7) beside
             native.rpn_proposals (A = 12, nms_pre 6000, nms_post 300) at 1, 4 and 15 frames of 38 x 63, on random maps.
  window     one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) of R-101 with a GARPNHead (synthetic
             GA-RPN weights, hvrnet_amd.synthetic.synth_ga_rpn_state_dict) against the stock RPNHead, alternating --reps times; with
             the kept fraction and the largest |shape delta| x std on the synthetic clip (the anchoring clip is at 13.8).
             --no-window skips it.

    python tools/ga_rpn_bench.py [--iters 30] [--out profiles/ga_rpn_bench.txt]

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
from hvrnet_amd.box_ops import AnchorGenerator  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tools.gconv_bench import DEV, FRAMES, LLC_BYTES, Report, timed  # noqa: E402

MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
H, W, C = 38, 63, 1024
FRACTIONS = (1.0, 0.3, 0.05)
GA_HEAD = dict(type='GARPNHead', in_channels=1024, feat_channels=1024, octave_base_scale=8, scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0],
               anchor_strides=[16], anchoring_stds=[0.07, 0.07, 0.14, 0.14], target_stds=[0.07, 0.07, 0.11, 0.11], loc_filter_thr=0.01)


def fmt(t):
    return '%7.1f us (%.1f, %.1f)' % (t[0], t[1], t[2])


def heads_report(args, lines, js):
    lines.append('masked heads (1 + 4 outputs, 1x1, K = %d) on %d frames of %d x %d beside the dense heads (5 rows padded to 8, f32 out);' % (C, FRAMES, H, W))
    lines.append('us per call, median (min, max) of %d groups; bytes = the kept rows of x + the keep map + the outputs, derived from the shapes' % args.iters)
    for mname, dt in MODES:
        gen = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn((FRAMES, H, W, C), generator=gen, device=DEV).clamp(min=0).to(dt)
        nbytes = x.numel() * x.element_size()
        n = max(2, min(8, int(2 * LLC_BYTES // nbytes) + 1))
        xs = [x] + [x.clone() for _ in range(n - 1)]
        w5 = (torch.randn((5, 1, 1, C), generator=gen, device=DEV) / C ** 0.5).to(dt)
        w8 = torch.zeros((8, 1, 1, C), dtype=dt, device=DEV)
        w8[:5] = w5
        b5, b8 = torch.zeros(5, device=DEV), torch.zeros(8, device=DEV)
        keeps = [(torch.rand((FRAMES, H, W), generator=gen, device=DEV) < f).to(torch.uint8) for f in FRACTIONS]
        o5 = torch.empty((FRAMES, H, W, 5), device=DEV)
        o8 = torch.empty((FRAMES, H, W, 8), device=DEV)
        calls = [lambda i, k=k: native.masked_conv2d_nhwc(xs[i % n], w5, b5, k, out=o5) for k in keeps]
        calls.append(lambda i: native.conv2d_nhwc(xs[i % n], w8, b8, relu=False, out_f32=True, out=o8))
        t = timed(calls, args.iters, args.group)
        dense = t[-1]
        P = FRAMES * H * W
        row = []
        for f, k, tm in zip(FRACTIONS, keeps, t):
            kept = int(k.sum())
            by = kept * C * x.element_size() + P * (1 + 20)
            row.append('kept %.2f %s %5.2f TB/s' % (f, fmt(tm), by / tm[0] / 1e6))
            js['heads %s kept %.2f us' % (mname, f)] = tm[0]
        lines.append('  %-4s %s   dense %s' % (mname, '   '.join(row), fmt(dense)))
        lines.append('       masked at 1.0 / dense = %.2f   masked at 0.3 / masked at 1.0 = %.2f   masked at 0.05 / masked at 1.0 = %.2f'
                     % (t[0][0] / dense[0], t[1][0] / t[0][0], t[2][0] / t[0][0]))
        js['heads %s dense us' % mname] = dense[0]
        js['heads %s masked_full_over_dense' % mname] = t[0][0] / dense[0]
        js['heads %s masked_0.3_over_full' % mname] = t[1][0] / t[0][0]
        del xs
        torch.cuda.empty_cache()


def mask_report(args, lines, js):
    gen = torch.Generator(device=DEV).manual_seed(2)
    ls = torch.randn((FRAMES, H, W, 4), generator=gen, device=DEV)
    w = torch.randn((72, 2), generator=gen, device=DEV) * 0.1
    keep = torch.empty((FRAMES, H, W), dtype=torch.uint8, device=DEV)
    om = torch.empty((FRAMES, H, W, 72), device=DEV)
    t, = timed([lambda i: native.ga_mask_offsets(loc=ls[..., 0:1], loc_filter_thr=0.5, shape=ls[..., 1:3], w_off=w, keep=keep, om=om)], args.iters, args.group)
    lines.append('mask + offsets (keep map and 72 offset channels) on %d frames of %d x %d: %s' % (FRAMES, H, W, fmt(t)))
    js['mask_offsets us'] = t[0]


def proposals_report(args, lines, js):
    lines.append('proposals on random maps of %d x %d: hvr_ga_rpn_proposals (kept 0.5, nms_pre 2000) beside hvr_rpn_proposals (A = 12, nms_pre 6000); nms_post = max_num = 300, thr 0.7' % (H, W))
    sq = AnchorGenerator(16, [8], [1.0]).base_anchors[0]
    gen12 = AnchorGenerator(16, [4, 8, 16, 32], [0.5, 1.0, 2.0])
    for T in (1, 4, 15):
        gen = torch.Generator(device=DEV).manual_seed(3)
        o = torch.randn((T, H, W, 8), generator=gen, device=DEV)
        o[..., 1:5] *= 2.0
        shape = torch.randn((T, H, W, 2), generator=gen, device=DEV) * 3.0
        keep = (torch.rand((T, H, W), generator=gen, device=DEV) < 0.5).to(torch.uint8)
        o12 = torch.randn((T, H, W, 60), generator=gen, device=DEV)
        ga = lambda i: native.ga_rpn_proposals(o[..., 0:1], o[..., 1:5], shape, keep, sq, 16, (0, 0, 0, 0), (0.07, 0.07, 0.14, 0.14), (0, 0, 0, 0),  # noqa: E731
                                               (0.07, 0.07, 0.11, 0.11), (600, 1000), 2000, 300, 300, 0.7)
        rp = lambda i: native.rpn_proposals(o12[..., :12], o12[..., 12:60], gen12.base_anchors, 16, (0, 0, 0, 0), (1, 1, 1, 1), (600, 1000),  # noqa: E731
                                            6000, 300, 300, 0.7)
        tg, tr = timed([ga, rp], args.iters, args.group)
        lines.append('  T = %2d   guided %s   RPNHead %s   guided / RPNHead = %.2f' % (T, fmt(tg), fmt(tr), tg[0] / tr[0]))
        js['proposals T=%d guided us' % T], js['proposals T=%d rpn us' % T] = tg[0], tr[0]


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which in ('RPNHead', 'GARPNHead'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        sd = S.synth_state_dict('hvr')
        if which == 'GARPNHead':
            cfg.model.rpn_head = GA_HEAD
            sd = {k: v for k, v in sd.items() if not k.startswith('rpn_head.')}
            sd.update(S.synth_ga_rpn_state_dict(1024, 4, GA_HEAD['loc_filter_thr']))
        model = hvrnet_amd.build_model(cfg, sd, torch.bfloat16, DEV)
        if which == 'GARPNHead':
            with torch.no_grad():
                c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
                outs = model.rpn_head([c4])
                _, counts = model.rpn_head.get_bboxes_batched(*outs, metas, model.test_cfg.rpn)
            keep = native.ga_loc_mask(outs[3][0].permute(0, 2, 3, 1), GA_HEAD['loc_filter_thr'])
            kept, big = float(keep.float().mean()), float((outs[2][0].abs().amax(dim=(0, 2, 3)).cpu() * torch.tensor(GA_HEAD['anchoring_stds'][2:])).max())
            lines.append('')
            lines.append('synthetic clip through the GARPNHead: kept fraction %.3f, largest |shape delta| x std %.2f (the clip is at 13.8), proposals per frame %d .. %d'
                         % (kept, big, int(counts.min()), int(counts.max())))
            js['kept fraction'], js['max shape x std'] = kept, big
        graphs[which] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the two heads alternating %d times:' % args.reps)
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
        sys.exit('ga_rpn_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/ga_rpn_bench.py on %s' % torch.cuda.get_device_name(0))
    heads_report(args, lines, js)
    mask_report(args, lines, js)
    proposals_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
