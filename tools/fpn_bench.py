"""Cost of the multi-level feature path (csrc/fpn.hip, hvrnet_amd/necks.py) on an otherwise idle MI355X, in one process, HIP-event times
(warm-up, then the median of --iters groups of --group back-to-back calls; the alternatives of a row take turns group by group, so
they see the same clocks):

  merge     hvr_fpn_merge on 15 frames of 152 x 256, 76 x 128, 38 x 64 and 19 x 32 maps with 256 channels (a 608 x 1024 frame at strides
            4 .. 32) in bf16, f16 and f32, beside the composite of the reference (per level an upsample and an in-place add, torch ops),
            with the byte model: every lateral read once, every output written once.
  extract   native.roi_align_levels at 15 x 300 and 15 x 1000 RoIs, C = 256, 7 x 7 bins, 2 x 2 samples, bf16 -- once with the RoIs spread
            evenly over the four levels, once with all of them on level 0 -- beside route='composite' (the reference's loop on the
            single-level call, host reads included: timed with a host clock around a synchronise) and beside the single-level call of
            equal K on the finest map.
  neck      the whole FPN (4 laterals, one merge, 4 3x3 convs, one subsampled level; bf16) behind ResNet-50 and ResNet-101 on the 15
            frames, beside the backbone's own time.  --no-neck skips it.

    python tools/fpn_bench.py [--iters 20] [--out profiles/fpn_bench.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvrnet_amd  # noqa: E402,F401
from hvrnet_amd import native, registry  # noqa: E402
from hvrnet_amd.backbone import set_compute_dtype  # noqa: E402

DEV = 'cuda:0'
HBM_PEAK = 8.0e12
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
B, C, P = 15, 256, 7
MAPS = [(152, 256), (76, 128), (38, 64), (19, 32)]
SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
IMG = (608, 1024)


class Report(list):
    """The report's lines, printed as they come (a run that ends early leaves what it measured)."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def timed_turns(fns, iters, group, warmup=3, host=False):
    """-> [(median, min, max) microseconds of one call] per function, the functions taking turns.  host: a host clock around a
    synchronise (for calls that read the host themselves) instead of HIP events."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            if host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(group):
                    fn()
                torch.cuda.synchronize()
                us[i].append((time.perf_counter() - t0) * 1e6 / group)
            else:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(group):
                    fn()
                e.record()
                torch.cuda.synchronize()
                us[i].append(s.elapsed_time(e) * 1e3 / group)
    return [(statistics.median(u), min(u), max(u)) for u in us]


def fmt(t):
    return '%8.1f us (min %.1f, max %.1f)' % t


def composite_merge(lats):
    """fpn.py:113-115 on NHWC maps: per level an upsample and an add (out of place on the first touch, so the inputs stay)."""
    m = [t for t in lats]
    for i in range(len(m) - 1, 0, -1):
        m[i - 1] = m[i - 1] + m[i].repeat_interleave(2, 1).repeat_interleave(2, 2)
    return m


def merge_report(args, lines, js):
    lines.append('merge (hvr_fpn_merge): %d frames of %s maps, %d channels; beside the composite (per level an upsample and an add, torch); '
                 'bytes = every lateral read once + every output written once' % (B, ' / '.join('%d x %d' % m for m in MAPS), C))
    for name, dt in MODES:
        g = torch.Generator().manual_seed(1)
        lats = [torch.randn((B, h, w, C), generator=g).to(DEV).to(dt) for h, w in MAPS]
        outs = [torch.empty_like(t) for t in lats[:-1]]
        nbytes = (sum(t.numel() for t in lats) + sum(o.numel() for o in outs)) * lats[0].element_size()
        t = timed_turns([lambda: native.fpn_merge(lats, out=outs), lambda: composite_merge(lats)], args.iters, args.group)
        lines.append('  %-4s one launch %s  %6.1f MB -> %5.2f TB/s (%4.1f %% of the 8 TB/s HBM peak)   composite %s  (x %.2f)' % (
            name, fmt(t[0]), nbytes / 1e6, nbytes / t[0][0] / 1e6, 100 * nbytes / t[0][0] * 1e6 / HBM_PEAK, fmt(t[1]), t[1][0] / t[0][0]))
        js['merge %s us' % name], js['merge %s composite us' % name] = t[0][0], t[1][0]
        del lats, outs


def level_rois(per_frame, spread, seed):
    """Seeded boxes on the 1024 x 608 image whose sizes put them evenly on the four levels of finest_scale 56 (spread) or all on level 0."""
    g = torch.Generator().manual_seed(seed)
    n = B * per_frame
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([float(IMG[1]), float(IMG[0])])
    if spread:
        lv = torch.arange(n) % 4
        side = 56.0 * (2.0 ** lv.float()) * (1.05 + 0.9 * torch.rand((n,), generator=g))     # inside [2^l, 2^(l+1)) x 56
    else:
        side = 16.0 + 90.0 * torch.rand((n,), generator=g)                                     # under 112 px
    half = side[:, None] / 2
    return torch.cat([torch.arange(B).repeat_interleave(per_frame)[:, None].float(), ctr - half, ctr + half - 1], 1)


def extract_report(args, lines, js):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(2)
    feats = [torch.randn((B, h, w, C), generator=g).to(DEV).to(dt) for h, w in MAPS]
    lines.append('')
    lines.append('extract (hvr_roi_align_levels_fwd): bf16, %d channels, %d x %d bins, 2 x 2 samples, four maps of %d frames; beside the composite (the loop '
                 'over the levels on the single-level call, host reads included; host clock) and the single-level call of equal K on the finest map' % (C, P, P, B))
    for per in (300, 1000):
        for spread in (True, False):
            rois = level_rois(per, spread, 10 + per).to(DEV).contiguous()
            K = rois.shape[0]
            out = torch.empty((K, P, P, C), dtype=dt, device=DEV)
            lv = native.roi_align_levels(feats, rois, P, SCALES, with_levels=True)[1]
            counts = np.bincount(lv.cpu().numpy(), minlength=4).tolist()
            one = lambda: native.roi_align_levels(feats, rois, P, SCALES, out=out)
            comp = lambda: native.roi_align_levels(feats, rois, P, SCALES, out=out, route='composite')
            single = lambda: native.roi_align_fwd(feats[0], rois, P, P, SCALES[0], 2, native.LAYOUT_NHWC, out=out)
            t = timed_turns([one, single], args.iters, args.group)
            th = timed_turns([one, comp], args.iters, max(1, args.group // 2), host=True)
            nbytes = out.numel() * 2 + sum(f.numel() for f in feats) * 2
            tag = '%d x %d RoIs, %s (levels %s)' % (B, per, 'even spread' if spread else 'all on level 0', counts)
            lines.append('  %s:' % tag)
            lines.append('    one launch   %s  maps + result %6.1f MB -> %5.2f TB/s' % (fmt(t[0]), nbytes / 1e6, nbytes / t[0][0] / 1e6))
            lines.append('    single level %s  (x %.2f of the one launch)' % (fmt(t[1]), t[1][0] / t[0][0]))
            lines.append('    host clock: one launch %s   composite %s  (x %.2f)' % (fmt(th[0]), fmt(th[1]), th[1][0] / th[0][0]))
            key = '%d %s' % (per, 'spread' if spread else 'level0')
            js['extract %s us' % key], js['extract %s single us' % key] = t[0][0], t[1][0]
            js['extract %s host us' % key], js['extract %s composite host us' % key] = th[0][0], th[1][0]


def neck_report(args, lines, js):
    lines.append('')
    lines.append('neck: FPN(in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5), bf16, behind the backbone on %d frames of %d x %d' % (B, IMG[0], IMG[1]))
    img = torch.randn((B, 3) + IMG, generator=torch.Generator().manual_seed(3)).to(DEV)
    for depth in (50, 101):
        bb = registry.build_backbone(dict(type='ResNet', depth=depth, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch'))
        neck = registry.build_neck(dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5))
        neck.init_weights()
        for m in (bb, neck):
            m.eval().to(DEV)
            set_compute_dtype(m, torch.bfloat16)
        with torch.no_grad():
            c = bb(img)
            t = timed_turns([lambda: bb(img), lambda: neck(c)], max(3, args.iters // 4), 1)
            native.profile_begin(tags=('fpn_merge',))
            neck(c)
            prof = native.profile_end()
        lines.append('  R-%d: backbone %s   neck %s  (%.1f %% of the backbone; the merge launch %.1f us of it)' % (
            depth, fmt(t[0]), fmt(t[1]), 100 * t[1][0] / t[0][0], prof['fpn_merge']['ms'] * 1e3))
        js['neck r%d backbone us' % depth], js['neck r%d us' % depth] = t[0][0], t[1][0]
        del bb, neck, c
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--group', type=int, default=10, help='calls between two events')
    ap.add_argument('--no-neck', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('fpn_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/fpn_bench.py on %s' % torch.cuda.get_device_name(0))
    merge_report(args, lines, js)
    extract_report(args, lines, js)
    if not args.no_neck:
        neck_report(args, lines, js)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
