"""Cost of RoI max pooling (csrc/roi_pool.hip, native.roi_pool_fwd / roi_pool_bwd, ops.RoIPool) on an otherwise idle MI355X, in one
process, HIP-event times (warm-up, then the median of --iters groups of --group back-to-back launches; RoIPool and RoIAlign take
turns group by group, so both see the same clocks):

  forward   hvr_roi_pool_fwd alone at the workload's shape -- 15 x 300 RoIs on the 256-channel 38 x 63 C5 map, 7 x 7 bins -- in bf16,
            f16 and f32, without and with the argmax, beside RoIAlign (2 x 2 samples) on the same map and RoIs, for three RoI
            populations: the window's own proposals on the synthetic clip, all whole-map RoIs, all RoIs under 32 px.  Beside every
            time two byte counts computed from the shapes: `unique` (the map once + the result and the argmax written once + the rois:
            what HBM must move if every re-read hits a cache) and `walked` (every pixel vector a lane asks for -- the bins' areas, from
            the header's f32 geometry, plus the first pixel of a bin once more -- and what it writes), and the rates they give.
  backward  hvr_roi_pool_bwd at 3 x 128 sampled RoIs (f32) beside hvr_roi_align_bwd, both with the zeroing of the gradient map.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, R101, hipGraph replay) with roi_layer RoIPool /
            RoIAlign, the two alternating --reps times.  --no-window skips it (the proposals are then seeded random boxes).

    python tools/roi_pool_bench.py [--iters 20] [--out profiles/roi_pool_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402

DEV = 'cuda:0'
HBM_PEAK = 8.0e12
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
B, H, W, C, NROI, P = 15, 38, 63, 256, 300, 7
SCALE = 1 / 16.0
T, HW, PAD = 15, (600, 1000), (608, 1008)


class Report(list):
    """The report's lines, printed as they come (a run that ends early leaves what it measured)."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def timed_turns(fns, iters, group, warmup=3):
    """-> [(median, min, max) microseconds of one call] per function: per iteration every function gets one group of `group` calls
    between two events, in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(group):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[i].append(s.elapsed_time(e) * 1e3 / group)
    return [(statistics.median(u), min(u), max(u)) for u in us]


def random_rois(frames, per_frame, lo, hi, seed):
    """Seeded boxes with sides in [lo, hi) px, centred anywhere on the 1000 x 600 image."""
    g = torch.Generator().manual_seed(seed)
    n = frames * per_frame
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([1000.0, 600.0])
    wh = torch.rand((n, 2), generator=g) * (hi - lo) + lo
    return torch.cat([torch.arange(frames).repeat_interleave(per_frame)[:, None].float(), ctr - wh / 2, ctr + wh / 2], 1)


def walked_pixels(rois):
    """Pixel vectors the forward kernel loads for these RoIs: the bins' areas by the header's rule (numpy f32, one rounding per
    operation) plus one more for every non-empty bin (its first pixel seeds the maximum)."""
    f = np.float32
    r = rois.cpu().numpy().astype(f)
    s = f(SCALE)
    rx1, ry1 = r[:, 1] * s, r[:, 2] * s
    rx2, ry2 = (r[:, 3] + f(1)) * s, (r[:, 4] + f(1)) * s
    rw, rh = rx2 - rx1, ry2 - ry1
    ok = (rw > 0) & (rh > 0) & (r[:, 0] >= 0) & (r[:, 0] < B)
    bw, bh = rw / f(P), rh / f(P)
    nx = np.stack([np.clip(np.ceil(f(p + 1) * bw + rx1), 0, W) - np.clip(np.floor(f(p) * bw + rx1), 0, W) for p in range(P)], 1)
    ny = np.stack([np.clip(np.ceil(f(p + 1) * bh + ry1), 0, H) - np.clip(np.floor(f(p) * bh + ry1), 0, H) for p in range(P)], 1)
    nx, ny = np.maximum(nx, 0) * ok[:, None], np.maximum(ny, 0) * ok[:, None]
    area = ny[:, :, None] * nx[:, None, :]
    return float(area.sum() + (area > 0).sum()), float(area[area > 0].mean()) if (area > 0).any() else 0.0


def forward_report(args, lines, js, proposals, proposals_name):
    n = B * NROI
    pops = [(proposals_name, proposals),
            ('whole-map RoIs', torch.cat([torch.arange(B).repeat_interleave(NROI)[:, None].float(), torch.tensor([[0.0, 0.0, 1007.0, 607.0]]).expand(n, 4)], 1)),
            ('RoIs under 32 px', random_rois(B, NROI, 4.0, 32.0, 6))]
    lines.append('forward alone (hvr_roi_pool_fwd): %d x %d RoIs on the %d-channel %d x %d map, %d x %d bins, beside RoIAlign (2 x 2 samples), taking turns;' % (
        B, NROI, C, H, W, P, P))
    lines.append('unique bytes = map + result (+ argmax) + rois once; walked bytes = every pixel vector loaded + everything written')
    for pname, rois in pops:
        assert tuple(rois.shape) == (n, 5)
        rois = rois.to(DEV).contiguous()
        px, mean_area = walked_pixels(rois)
        lines.append('  %s (mean non-empty bin %.1f px, %.0f pixel vectors walked):' % (pname, mean_area, px))
        for mname, dt in MODES:
            x = torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(1)).to(DEV).to(dt)
            es = x.element_size()
            out = torch.empty((n, P, P, C), dtype=dt, device=DEV)
            oa = torch.empty((n, P, P, C), dtype=dt, device=DEV)
            t = timed_turns([lambda: native.roi_pool_fwd(x, rois, P, P, SCALE, out=out),
                             lambda: native.roi_pool_fwd(x, rois, P, P, SCALE, with_argmax=True, out=out),
                             lambda: native.roi_align_fwd(x, rois, P, P, SCALE, 2, native.LAYOUT_NHWC, out=oa)], args.iters, args.group)
            for form, tt, extra in (('no argmax', t[0], 0), ('argmax', t[1], n * P * P * C * 4)):
                unique = x.numel() * es + out.numel() * es + extra + rois.numel() * 4
                walked = px * C * es + out.numel() * es + extra
                side = 'faster than' if tt[0] < t[2][0] else 'slower than'
                lines.append('    %-4s RoIPool %-9s %8.1f us (min %.1f, max %.1f)  unique %5.1f MB -> %5.2f TB/s (%4.1f %% of the 8 TB/s HBM peak)  walked %7.1f MB -> %5.2f TB/s'
                             '   %s RoIAlign (x %.2f)' % (mname, form, tt[0], tt[1], tt[2], unique / 1e6, unique / tt[0] / 1e6, 100 * unique / tt[0] * 1e6 / HBM_PEAK,
                                                         walked / 1e6, walked / tt[0] / 1e6, side, tt[0] / t[2][0]))
                js['fwd %s %s %s us' % (pname, mname, form)] = tt[0]
            gather = n * P * P * (16 + 1) * C * es
            lines.append('    %-4s RoIAlign          %8.1f us (min %.1f, max %.1f)  gather %7.1f MB -> %5.2f TB/s' % (mname, t[2][0], t[2][1], t[2][2], gather / 1e6,
                                                                                                                 gather / t[2][0] / 1e6))
            js['fwd %s %s roi_align us' % (pname, mname)] = t[2][0]
            del x, out, oa


def backward_report(args, lines, js):
    frames, per = 3, 128
    n = frames * per
    rois = random_rois(frames, per, 16.0, 316.0, 4).to(DEV).contiguous()
    x = torch.randn((frames, H, W, C), generator=torch.Generator().manual_seed(2)).to(DEV)
    go = torch.randn((n, P, P, C), generator=torch.Generator().manual_seed(3)).to(DEV)
    _, arg = native.roi_pool_fwd(x, rois, P, P, SCALE, with_argmax=True)
    shape = (frames, H, W, C)
    t = timed_turns([lambda: native.roi_pool_bwd(go, rois, arg, shape),
                     lambda: native.roi_align_bwd(go, rois, shape, SCALE, 2, native.LAYOUT_NHWC)], args.iters, args.group)
    read = go.numel() * 4 + arg.numel() * 4
    lines.append('')
    lines.append('backward (f32, %d x %d sampled RoIs, the %d x %d x %d x %d gradient map zeroed in the call), taking turns:' % (frames, per, frames, H, W, C))
    lines.append('  RoIPool   %8.1f us (min %.1f, max %.1f)  grad_out + argmax read %5.1f MB -> %5.2f TB/s, %d atomics   %s RoIAlign (x %.2f)' % (
        t[0][0], t[0][1], t[0][2], read / 1e6, read / t[0][0] / 1e6, int((arg >= 0).sum()), 'faster than' if t[0][0] < t[1][0] else 'slower than', t[0][0] / t[1][0]))
    lines.append('  RoIAlign  %8.1f us (min %.1f, max %.1f)  grad_out read %5.1f MB -> %5.2f TB/s' % (t[1][0], t[1][1], t[1][2], go.numel() * 4 / 1e6,
                                                                                                   go.numel() * 4 / t[1][0] / 1e6))
    js['bwd roi_pool us'], js['bwd roi_align us'] = t[0][0], t[1][0]


def window_models():
    models = {}
    for layer_type in ('RoIPool', 'RoIAlign'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=NROI)
        if layer_type == 'RoIPool':
            cfg.model.bbox_roi_extractor['roi_layer'] = dict(type='RoIPool', out_size=P)
        models[layer_type] = hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr'), torch.bfloat16, DEV)
    return models


def window_report(args, lines, js, models, clip, metas):
    from hvrnet_amd.graphs import GraphedClip
    graphs = {name: GraphedClip(m, clip, metas, rescale=True) for name, m in models.items()}
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, R101 + HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the two roi_layers alternating %d times:' % args.reps)
    for rep in range(args.reps):
        row = []
        for name, g in graphs.items():
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
            row.append((name, statistics.median(ms), min(ms), max(ms)))
            js.setdefault('window %s ms' % name, []).append(statistics.median(ms))
        lines.append('  round %d: ' % (rep + 1) + '   '.join('%s %.2f (min %.2f, max %.2f)' % r for r in row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--group', type=int, default=10, help='launches between two events')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('roi_pool_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/roi_pool_bench.py on %s' % torch.cuda.get_device_name(0))
    if args.no_window:
        proposals, pname = random_rois(B, NROI, 16.0, 316.0, 4), 'seeded random boxes of 16 - 316 px'
    else:
        models = window_models()
        metas = [S.synth_meta(HW, PAD) for _ in range(T)]
        clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
        with torch.no_grad():
            c4 = models['RoIPool'](img=clip, img_meta=metas, backbone_feat=True)[0]
            proposals = models['RoIPool'].window_tensors(c4, metas, speculate=True)['rois'].float().cpu()
        pname = "the window's own proposals on the synthetic clip"
        del c4
    forward_report(args, lines, js, proposals, pname)
    backward_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js, models, clip, metas)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
