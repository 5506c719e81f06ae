"""Cost of the deformable-conv path (csrc/dcn.hip, native.deform_im2col / deform_conv2d_nhwc) on an otherwise idle MI355X, in one
process, HIP-event times (warm-up, then the median of --iters groups of --group back-to-back launches):

  sampler   hvr_deform_im2col alone at the workload's shapes -- layer 3 (38 x 63, Cin 256, dilation 1) and res5 (38 x 63, Cin 512,
            dilation 2), modulated, one group, 15 and 60 frames, in each compute mode.  Beside every time two byte counts computed
            from the shapes: `unique` (x once + offsets once + col written once: what HBM must move if every corner re-read hits a
            cache) and `gather` (four corner vectors read + one written per output element: what the lanes ask for), and the rates
            they give, next to RoIAlign's gather rate at the workload's shape (15 frames x 300 RoIs on the 1024-channel C4 map,
            counted the same way: 16 corner vectors per bin + one written) and the 8 TB/s HBM peak (MI355X_MICROARCH).
  product   the GEMM on col (native.gemm, the deformable conv's second half) beside the plain implicit-GEMM 3x3 of the same shape
            (native.conv2d_nhwc), the offset conv, and the whole deform_conv2d_nhwc -- at 60 frames also per chunk size.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, R101, hipGraph replay) with dcn in layer 3 + res5,
            in res5 only, and without, the three alternating --reps times.  --no-window skips it.

    python tools/dcn_bench.py [--iters 20] [--out profiles/dcn_bench.txt]

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

DEV = 'cuda:0'
HBM_PEAK = 8.0e12
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f16x2', native.SPLIT), ('f32', torch.float32)]
SHAPES = [('layer3', 38, 63, 256, 1), ('res5', 38, 63, 512, 2)]


class Report(list):
    """The report's lines, printed as they come (a run that ends early leaves what it measured)."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def timed(fn, iters, group, warmup=3):
    """-> (median, min, max) microseconds of one call: `group` calls between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(group):
            fn()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) * 1e3 / group)
    return statistics.median(us), min(us), max(us)


def operand(shape, dtype, seed, relu=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    t = (t.clamp(min=0.0) if relu else t).to(DEV)
    return native.cast(t, native.SPLIT) if dtype == native.SPLIT else t.to(dtype)


def weight(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    fan = shape[1] * shape[2] * shape[3]
    return native.as_operand((torch.randn(shape, generator=g) / fan ** 0.5).to(DEV), dtype)


def offsets(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    om = torch.zeros((B, H, W, 28))
    om[..., :18] = torch.randn((B, H, W, 18), generator=g) * 1.5
    om[..., 18:27] = torch.randn((B, H, W, 9), generator=g) * 2.0
    return om.to(DEV)


def sampler_report(args, lines, js):
    lines.append('sampler alone (hvr_deform_im2col, modulated, 1 group, 3x3, stride 1; offsets N(0, 1.5) px): time per call,')
    lines.append('unique bytes = x + offsets + col once, gather bytes = 4 corner vectors read + 1 written per output element')
    for name, H, W, C, dil in SHAPES:
        for B in (15, 60):
            for mname, dt in MODES:
                x = operand((B, H, W, C), dt, 1)
                om = offsets(B, H, W, 2)
                M, K, es = B * H * W, 9 * C, x.element_size()
                col = torch.empty((M, K), dtype=x.dtype, device=DEV)
                t = timed(lambda: native.deform_im2col(x, om, 3, 3, 1, dil, dil, 1, True, out=col), args.iters, args.group)
                unique = x.numel() * es + om.numel() * 4 + M * K * es
                gather = 5 * M * K * es
                lines.append('  %-6s %2d frames %-5s %9.1f us (min %.1f, max %.1f)  col %6.1f MB  unique %6.1f MB -> %5.2f TB/s (%4.1f %% of the 8 TB/s HBM peak)  gather %7.1f MB -> %5.2f TB/s'
                             % (name, B, mname, t[0], t[1], t[2], M * K * es / 1e6, unique / 1e6, unique / t[0] / 1e6, 100 * unique / t[0] * 1e6 / HBM_PEAK,
                                gather / 1e6, gather / t[0] / 1e6))
                js['sampler %s B%d %s us' % (name, B, mname)] = t[0]
                del x, col
    # RoIAlign at the workload's shape, counted the same way
    feat = operand((15, 38, 63, 1024), torch.bfloat16, 3)
    g = torch.Generator().manual_seed(4)
    n = 15 * 300
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([1000.0, 600.0])
    wh = torch.rand((n, 2), generator=g) * 300 + 16
    rois = torch.cat([torch.arange(15).repeat_interleave(300)[:, None].float(), ctr - wh / 2, ctr + wh / 2], 1).to(DEV)
    t = timed(lambda: native.roi_align_fwd(feat, rois, 7, 7, 1 / 16.0, 2, native.LAYOUT_NHWC), args.iters, args.group)
    gather = n * 49 * (16 + 1) * 1024 * 2
    lines.append('  RoIAlign 15 x 300 RoIs, 7 x 7 x 2 x 2 samples, 1024 channels, bf16: %.1f us (min %.1f, max %.1f)  gather %.1f MB -> %.2f TB/s' % (
        t[0], t[1], t[2], gather / 1e6, gather / t[0] / 1e6))
    js['roi_align us'] = t[0]
    js['roi_align gather TB/s'] = gather / t[0] / 1e6


def product_report(args, lines, js):
    lines.append('')
    lines.append('the deformable conv\'s halves beside the plain 3x3 of the same shape (Cout = Cin, bias + ReLU):')
    for name, H, W, C, dil in SHAPES:
        for B in (15, 60):
            for mname, dt in MODES:
                x = operand((B, H, W, C), dt, 5)
                om = offsets(B, H, W, 6)
                w = weight((C, 3, 3, C), dt, 7)
                wo = weight((28, 3, 3, C), dt, 8)
                bias = torch.zeros(C, device=DEV)
                bo = torch.zeros(28, device=DEV)
                M, K = B * H * W, 9 * C
                if M * K * x.element_size() < 2 ** 31:
                    col = native.deform_im2col(x, om, 3, 3, 1, dil, dil, 1, True)
                    y = torch.empty((M, C), dtype=x.dtype, device=DEV)
                    tg = timed(lambda: native.gemm(col, w.reshape(C, K), bias, relu=True, out=y), args.iters, args.group)
                    del col, y
                else:   # (hvr_gemm takes operands below 2 GiB: deform_conv2d_nhwc never builds this col whole)
                    tg = (float('nan'),) * 3
                tc = timed(lambda: native.conv2d_nhwc(x, w, bias, relu=True, pad=dil, dil=dil), args.iters, args.group)
                to = timed(lambda: native.conv2d_nhwc(x, wo, bo, relu=False, pad=dil, dil=dil, out_f32=True), args.iters, args.group)
                td = timed(lambda: native.deform_conv2d_nhwc(x, om, w, bias, True, 1, dil, dil, 1, True), args.iters, max(1, args.group // 2))
                lines.append('  %-6s %2d frames %-5s  GEMM on col %8.1f us   plain 3x3 conv %8.1f us   offset conv (28 ch) %7.1f us   deform_conv2d_nhwc (sampler + GEMM, chunks of %d rows) %8.1f us'
                             % (name, B, mname, tg[0], tc[0], to[0], native.DEFORM_CHUNK_ROWS, td[0]))
                js['gemm_on_col %s B%d %s us' % (name, B, mname)] = tg[0]
                js['plain_conv %s B%d %s us' % (name, B, mname)] = tc[0]
                js['offset_conv %s B%d %s us' % (name, B, mname)] = to[0]
                js['deform_conv %s B%d %s us' % (name, B, mname)] = td[0]
                if B == 60 and mname == 'bf16':
                    for frames in (1, 4, 8, 15, 30, 60):
                        rows = frames * H * W
                        tt = timed(lambda: native.deform_conv2d_nhwc(x, om, w, bias, True, 1, dil, dil, 1, True, chunk_rows=rows), args.iters, max(1, args.group // 2))
                        lines.append('      chunk of %2d frames (%6d rows, col scratch %6.1f MB): %8.1f us' % (frames, rows, rows * K * 2 / 1e6, tt[0]))
                        js['deform_conv %s B60 bf16 chunk%d us' % (name, frames)] = tt[0]
                del x, w


def dcn_state_dict(where, seed=91):
    sd = S.synth_state_dict('hvr')
    g = torch.Generator().manual_seed(seed)
    stages = [('shared_head.layer4', 512, 3)] + ([('backbone.layer3', 256, 23)] if where == 'layer3+res5' else [])
    for prefix, planes, blocks in stages:
        for i in range(blocks):
            sd['%s.%d.conv2_offset.weight' % (prefix, i)] = torch.randn((27, planes, 3, 3), generator=g) * 0.02
            sd['%s.%d.conv2_offset.bias' % (prefix, i)] = torch.randn((27,), generator=g) * 0.3
    return sd


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = 15, (600, 1000), (608, 1008)
    dcn = dict(modulated=True, deformable_groups=1, fallback_on_stride=False)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for where in ('none', 'res5', 'layer3+res5'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        if where != 'none':
            cfg.model.shared_head['dcn'] = dcn
        if where == 'layer3+res5':
            cfg.model.backbone['dcn'] = dcn
            cfg.model.backbone['stage_with_dcn'] = (False, False, True)
        model = hvrnet_amd.build_model(cfg, S.synth_state_dict('hvr') if where == 'none' else dcn_state_dict(where), torch.bfloat16, DEV)
        graphs[where] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, R101 + HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the three models alternating %d times:' % args.reps)
    for rep in range(args.reps):
        row = []
        for where, g in graphs.items():
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
            row.append((where, statistics.median(ms), min(ms), max(ms)))
            js.setdefault('window %s ms' % where, []).append(statistics.median(ms))
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
        sys.exit('dcn_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/dcn_bench.py on %s' % torch.cuda.get_device_name(0))
    sampler_report(args, lines, js)
    product_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
