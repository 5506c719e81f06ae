"""Cost of deformable RoI pooling (csrc/dpool.hip, native.deform_roi_pool, ops.DeformRoIPoolingPack / ModulatedDeformRoIPoolingPack)
on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then the median of --iters groups of --group back-to-back
launches):

  kernel    hvr_deform_roi_pool_fwd alone at the workload's shape -- 15 x 300 RoIs on the 256-channel 38 x 63 C5 map, 7 x 7 bins of
            4 x 4 samples -- in each compute mode, pass 1 (no offsets) and pass 2 (offsets N(0, 3) x trans_std 0.1, mask logits),
            beside RoIAlign (2 x 2 samples) on the same map and RoIs.  Beside every time two byte counts computed from the shapes:
            `unique` (the map once + the result written once + rois / offsets / logits once: what HBM must move if every corner
            re-read hits a cache) and `gather` (4 spp^2 corner vectors read + one written per bin: what the lanes ask for at most --
            skipped samples are counted), and the rates they give.
  chain     the offset / mask FC chain of the stock packs (deform_fc_channels 1024) on 4 500 pooled rows: the fused first layer
            (2 x 1024 outputs, K = 12 544), the two first layers as separate GEMMs, the remaining layers, and the whole pack forward.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, R101, hipGraph replay) with roi_layer RoIAlign /
            DeformRoIPoolingPack / ModulatedDeformRoIPoolingPack, the three alternating --reps times.  --no-window skips it.

    python tools/dpool_bench.py [--iters 20] [--out profiles/dpool_bench.txt]

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
from hvrnet_amd import backbone, native, ops, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402

DEV = 'cuda:0'
HBM_PEAK = 8.0e12
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f16x2', native.SPLIT), ('f32', torch.float32)]
B, H, W, C, NROI, P, SPP = 15, 38, 63, 256, 300, 7, 4
SCALE, TRANS_STD = 1 / 16.0, 0.1


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


def operand(shape, dtype, seed):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).clamp(min=0.0).to(DEV)
    return native.cast(t, native.SPLIT) if dtype == native.SPLIT else t.to(dtype)


def workload_rois(seed=4):
    g = torch.Generator().manual_seed(seed)
    n = B * NROI
    ctr = torch.rand((n, 2), generator=g) * torch.tensor([1000.0, 600.0])
    wh = torch.rand((n, 2), generator=g) * 300 + 16
    return torch.cat([torch.arange(B).repeat_interleave(NROI)[:, None].float(), ctr - wh / 2, ctr + wh / 2], 1).to(DEV)


def kernel_report(args, lines, js):
    n = B * NROI
    lines.append('kernel alone (hvr_deform_roi_pool_fwd): %d x %d RoIs on the %d-channel %d x %d map, %d x %d bins, %d x %d samples per bin;' % (B, NROI, C, H, W, P, P, SPP, SPP))
    lines.append('unique bytes = map + result + rois / offsets / logits once, gather bytes = (4 spp^2 corner vectors + 1 written) per bin')
    rois = workload_rois()
    g = torch.Generator().manual_seed(5)
    wide_t = (torch.randn((n, 100), generator=g) * 3.0).to(DEV)
    wide_m = (torch.randn((n, 52), generator=g) * 2.0).to(DEV)
    trans, mask = wide_t[:, :2 * P * P], wide_m[:, :P * P]
    for mname, dt in MODES:
        x = operand((B, H, W, C), dt, 1)
        es = x.element_size()
        out = None if dt == native.SPLIT else torch.empty((n, P, P, C), dtype=dt, device=DEV)
        for pname, t_, m_ in (('pass 1 (no offsets)', None, None), ('pass 2 (offsets)', trans, None), ('pass 2 (offsets + mask)', trans, mask)):
            t = timed(lambda: native.deform_roi_pool(x, rois, t_, m_, P, C, 1, P, SPP, SCALE, TRANS_STD, out=out), args.iters, args.group)
            small = rois.numel() * 4 + (0 if t_ is None else n * 98 * 4) + (0 if m_ is None else n * 49 * 4)
            unique = x.numel() * es + n * P * P * C * es + small
            gather = n * P * P * (4 * SPP * SPP + 1) * C * es
            lines.append('  %-5s %-24s %8.1f us (min %.1f, max %.1f)  unique %5.1f MB -> %5.2f TB/s (%4.1f %% of the 8 TB/s HBM peak)  gather %7.1f MB -> %5.2f TB/s'
                         % (mname, pname, t[0], t[1], t[2], unique / 1e6, unique / t[0] / 1e6, 100 * unique / t[0] * 1e6 / HBM_PEAK, gather / 1e6,
                            gather / t[0] / 1e6))
            js['kernel %s %s us' % (mname, pname)] = t[0]
        oa = None if dt == native.SPLIT else torch.empty((n, P, P, C), dtype=dt, device=DEV)
        t = timed(lambda: native.roi_align_fwd(x, rois, P, P, SCALE, 2, native.LAYOUT_NHWC, out=oa), args.iters, args.group)
        gather = n * P * P * (16 + 1) * C * es
        lines.append('  %-5s %-24s %8.1f us (min %.1f, max %.1f)  gather %7.1f MB -> %5.2f TB/s' % (mname, 'RoIAlign, 2 x 2 samples', t[0], t[1], t[2],
                                                                                                  gather / 1e6, gather / t[0] / 1e6))
        js['roi_align %s us' % mname] = t[0]
        del x, out, oa


def randomise(pack, seed):
    g = torch.Generator().manual_seed(seed)
    for name in ('offset_fc', 'mask_fc'):
        fcs = [m for m in getattr(pack, name, ()) if isinstance(m, torch.nn.Linear)]
        for i, fc in enumerate(fcs):
            std = (1.0 / fc.in_features) ** 0.5 * (3.0 if i == len(fcs) - 1 else 1.4)
            fc.weight.data = torch.randn(fc.weight.shape, generator=g) * std
            fc.bias.data = torch.randn(fc.bias.shape, generator=g) * 0.1
    return pack


def chain_report(args, lines, js):
    n = B * NROI
    lines.append('')
    lines.append('the FC chain of the stock packs on %d pooled rows (K = %d, deform_fc_channels 1024), and the whole pack forward:' % (n, P * P * C))
    rois = workload_rois()
    for mname, dt in MODES:
        x = operand((B, H, W, C), dt, 1)
        v2 = randomise(ops.ModulatedDeformRoIPoolingPack(SCALE, P, C, False, trans_std=TRANS_STD), 7).to(DEV).eval()
        v1 = randomise(ops.DeformRoIPoolingPack(SCALE, P, C, False, trans_std=TRANS_STD), 8).to(DEV).eval()
        backbone.set_compute_dtype(v2, dt)
        backbone.set_compute_dtype(v1, dt)
        with torch.no_grad():
            p = v2.packed(torch.device(DEV))
            f = native.cast(x, torch.float32) if dt == native.SPLIT else x
            rows = native.deform_roi_pool(f, rois, None, None, P, C, 1, P, SPP, SCALE, TRANS_STD).view(n, -1)
            rows = native.cast(rows, dt) if dt == native.SPLIT else rows
            wf, bf = p['fused0']
            tf = timed(lambda: native.gemm(rows, wf, bf, relu=True), args.iters, args.group)
            wo, bo, wm, bm = wf[:1024], bf[:1024], wf[1024:], bf[1024:]
            ts = timed(lambda: (native.gemm(rows, wo, bo, relu=True), native.gemm(rows, wm, bm, relu=True)), args.iters, args.group)
            h = native.gemm(rows, wf, bf, relu=True)
            tr = timed(lambda: (v2._chain(p['off'], h[:, :1024], 1), v2._chain(p['mask'], h[:, 1024:], 1)), args.iters, args.group)
            xl = backbone.as_logical(x)
            t2 = timed(lambda: v2(xl, rois), args.iters, max(1, args.group // 2))
            t1 = timed(lambda: v1(xl, rois), args.iters, max(1, args.group // 2))
        flop = 2.0 * n * P * P * C * 2048
        lines.append('  %-5s fused first layer %8.1f us (%.0f TF/s)   as two GEMMs %8.1f us   remaining layers (1024 -> 1024 -> 100, 1024 -> 52) %7.1f us   '
                     'ModulatedDeformRoIPoolingPack forward %8.1f us   DeformRoIPoolingPack forward %8.1f us'
                     % (mname, tf[0], flop / tf[0] / 1e6, ts[0], tr[0], t2[0], t1[0]))
        for k, v in (('fused0', tf), ('two_gemms', ts), ('rest', tr), ('v2_forward', t2), ('v1_forward', t1)):
            js['chain %s %s us' % (mname, k)] = v[0]
        del v1, v2, p, x, rows, h


def pool_state_dict(layer_type, seed=91):
    sd = S.synth_state_dict('hvr')
    if layer_type != 'RoIAlign':
        pack = randomise(getattr(ops, layer_type)(SCALE, P, C, False, trans_std=TRANS_STD), seed)
        for k, v in pack.state_dict().items():
            sd['bbox_roi_extractor.roi_layers.0.' + k] = v
    return sd


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = 15, (600, 1000), (608, 1008)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for layer_type in ('RoIAlign', 'DeformRoIPoolingPack', 'ModulatedDeformRoIPoolingPack'):
        cfg = hvr_config(frame_interval=T // 2, nms_post=NROI)
        if layer_type != 'RoIAlign':
            cfg.model.bbox_roi_extractor['roi_layer'] = dict(type=layer_type, out_size=P, out_channels=C, no_trans=False, group_size=1,
                                                             trans_std=TRANS_STD)
        model = hvrnet_amd.build_model(cfg, pool_state_dict(layer_type), torch.bfloat16, DEV)
        graphs[layer_type] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, R101 + HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the three roi_layers alternating %d times:' % args.reps)
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
        sys.exit('dpool_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/dpool_bench.py on %s' % torch.cuda.get_device_name(0))
    kernel_report(args, lines, js)
    chain_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
