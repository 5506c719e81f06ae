"""Cost of the generalized attention core (csrc/gen_attn.hip) on an otherwise idle MI355X, in one process, HIP-event times (warm-up, then
the median of --iters groups of back-to-back launches; the calls that are compared at one shape take turns group by group, so that a
drift of the clocks or a neighbour on the host meets all of them alike -- tools/gconv_bench.py's method):

  core      native.gen_attention, type '1111', 8 heads, kv_stride 2, on 15 frames of the layer-2 map (76 x 126 queries, 38 x 63 keys,
            d = 16) and of the layer-3 map (38 x 63 queries, 19 x 32 keys, d = 32): the kernel route in bf16 and half beside the
            composite route (the reference's matmul / softmax / matmul in f32 over chunks of rows, energy buffer capped at
            native.GEN_ATTN_ENERGY_CAP) in bf16, half and f32 (split half runs the f32 form), and beside the reference's formulation
            left in the map's own format ('torch', what a PyTorch user of the reference's module gets under autocast: it holds the
            whole energy tensor, so it is measured where that fits in --torch-cap bytes, on fewer frames and scaled if need be).
            Milliseconds, and the fraction of the mode's dense MFMA peak with 4 P Mk d flop per head and frame (2.5 PF for bf16 and
            half, 157 TF for f32: the figures of the microarchitecture notes; no counter was read).
  one row   type '0010' (energies that do not depend on the query): the one-row call, kernel beside composite, at both key grids.
  window    one clip window (T = 15, 608 x 1008, 300 proposals, bf16 HVR head, hipGraph replay) of R-101 with '1111' attention in
            every block of layer 3, and of layers 2 and 3, beside the plain R-101 (the benchmark's model), alternating --reps
            times.  --no-window skips it.

    python tools/gen_attention_bench.py [--iters 20] [--out profiles/gen_attention_bench.txt]

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
from tools.gconv_bench import DEV, FRAMES, Report, timed  # noqa: E402

SHAPES = [('layer2', 76, 126, 16), ('layer3', 38, 63, 32)]
HEADS, STRIDE = 8, 2
PEAK = {'bf16': 2.5e15, 'f16': 2.5e15, 'f32': 157.3e12}
MODES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]


def operands(B, H, W, d, dt, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    Hk, Wk = (H - 1) // STRIDE + 1, (W - 1) // STRIDE + 1
    n = lambda *s: torch.randn(s, generator=g, device=DEV)   # noqa: E731
    sc = d ** -0.25
    return dict(q=(n(B, H * W, HEADS * d) * sc).to(dt), k=(n(B, Hk * Wk, HEADS * d) * sc).to(dt), v=n(B, Hk * Wk, HEADS * d).to(dt),
                ab=(n(HEADS * d) * sc).contiguous(), px=(n(HEADS, W, Wk, d) * sc * 0.7).to(dt), py=(n(HEADS, H, Hk, d) * sc * 0.7).to(dt),
                gx=n(HEADS, W, Wk).contiguous(), gy=n(HEADS, H, Hk).contiguous(), H=H, W=W, Hk=Hk, Wk=Wk, d=d)


def core(c, route):
    return native.gen_attention(c['q'], c['k'], c['v'], HEADS, c['d'], c['H'], c['W'], c['Hk'], c['Wk'], appr_bias=c['ab'], px=c['px'], py=c['py'],
                                gx=c['gx'], gy=c['gy'], qk=True, route=route)


def torch_formulation(c):
    """generalized_attention.py:268-368 for '1111' in the operands' own format: (q + appr_bias) k, the two position products with
    (q + geom_bias) folded as here (q . P + G), one energy tensor, softmax, matmul."""
    B, d, H, W, Hk, Wk = c['q'].shape[0], c['d'], c['H'], c['W'], c['Hk'], c['Wk']
    dt = c['q'].dtype
    q = c['q'].view(B, H * W, HEADS, d).permute(0, 2, 1, 3)
    kT = c['k'].view(B, Hk * Wk, HEADS, d).permute(0, 2, 3, 1)
    v = c['v'].view(B, Hk * Wk, HEADS, d).permute(0, 2, 1, 3)
    e = torch.matmul(q + c['ab'].to(dt).view(1, HEADS, 1, d), kT).view(B, HEADS, H, W, Hk, Wk)
    q5 = q.reshape(B, HEADS, H, W, d)
    ex = torch.matmul(q5.permute(0, 1, 3, 2, 4), c['px'].permute(0, 1, 3, 2).unsqueeze(0)).permute(0, 1, 3, 2, 4) + c['gx'].to(dt).view(1, HEADS, 1, W, Wk)
    ey = torch.matmul(q5, c['py'].permute(0, 1, 3, 2).unsqueeze(0)) + c['gy'].to(dt).view(1, HEADS, H, 1, Hk)
    e = e + ex.unsqueeze(4) + ey.unsqueeze(5)
    a = torch.softmax(e.view(B, HEADS, H * W, Hk * Wk), 3)
    return torch.matmul(a, v).permute(0, 2, 1, 3).reshape(B, H * W, HEADS * d)


def core_report(args, lines, js):
    lines.append("the attention core, type '1111', %d heads, kv_stride %d, %d frames; ms per call, median (min, max) of %d groups; peak = 4 P Mk d flop" % (HEADS, STRIDE, FRAMES, args.iters))
    lines.append('per head and frame over the time, as a fraction of the dense MFMA peak of the mode (bf16 / half 2.5 PF, f32 157 TF)')
    for name, H, W, d in SHAPES:
        for mname, dt in MODES:
            c = operands(FRAMES, H, W, d, dt)
            P, Mk = H * W, c['Hk'] * c['Wk']
            flop = 4.0 * P * Mk * d * HEADS * FRAMES
            energy = FRAMES * HEADS * P * Mk * (2 if dt != torch.float32 else 4)
            bt = FRAMES
            while bt > 1 and 3 * bt * HEADS * P * Mk * c['q'].element_size() > args.torch_cap:      # (energy, its softmax, and a temporary of the sum)
                bt -= 1
            fits = 3 * bt * HEADS * P * Mk * c['q'].element_size() <= args.torch_cap
            ct = operands(bt, H, W, d, dt) if fits else None
            calls, tags = [], []
            if native.gen_attn_supported(d, HEADS, c['Hk'], c['Wk'], dt):
                calls.append(lambda i: core(c, 'kernel'))
                tags.append('kernel')
            calls.append(lambda i: core(c, 'composite'))
            tags.append('composite')
            if fits:
                calls.append(lambda i: torch_formulation(ct))
                tags.append('torch')
            res = timed(calls, args.iters, args.group)
            head = '  %-7s %3dx%-3d queries %2dx%-2d keys d %2d %-4s' % (name, H, W, c['Hk'], c['Wk'], d, mname)
            row = []
            for tag, (med, lo, hi) in zip(tags, res):
                scale = FRAMES / bt if tag == 'torch' else 1.0
                ms = med * scale / 1e3
                row.append('%s %8.3f ms (%.3f, %.3f) %5.1f %% of peak' % (tag if scale == 1.0 else 'torch (%d frames x %.2f)' % (bt, scale), ms, lo * scale / 1e3,
                                                                          hi * scale / 1e3, 100.0 * flop / (ms * 1e-3) / PEAK[mname]))
                js['%s %s %s ms' % (name, mname, tag)] = ms
            if not fits:
                row.append('torch: the energy tensor of ONE frame, %.1f GB with its softmax, is over the cap' % (3 * HEADS * P * Mk * c['q'].element_size() / 1e9))
            lines.append(head + '  ' + '   '.join(row))
            lines.append(' ' * len(head) + '  (the energy tensor the reference holds: %.2f GB; automatic route: %s)'
                         % (energy / 1e9, native.gen_attn_route(d, HEADS, H, W, c['Hk'], c['Wk'], dt)))
            if 'kernel' in tags:
                js['%s %s kernel over composite' % (name, mname)] = res[0][0] / res[1][0]
            del c, ct
            torch.cuda.empty_cache()


def one_row_report(args, lines, js):
    """Type '0010': the energies do not depend on the query, the core is called for ONE row per frame and head (H = W = 1)."""
    lines.append('')
    lines.append("type '0010', the one-row call (a single query per frame and head; grid (1, heads, frames)), us per call, median (min, max):")
    for name, H, W, d in SHAPES:
        for mname, dt in MODES[:2]:
            c = operands(FRAMES, H, W, d, dt)
            call = lambda route: native.gen_attention(None, c['k'], c['v'], HEADS, d, 1, 1, c['Hk'], c['Wk'], appr_bias=c['ab'], qk=False, route=route)   # noqa: E731
            (tk, tc) = timed([lambda i: call('kernel'), lambda i: call('composite')], args.iters, args.group)
            lines.append('  %-7s %2dx%-2d keys d %2d %-4s  kernel %7.1f us (%.1f, %.1f)   composite %7.1f us (%.1f, %.1f)   automatic route: %s'
                         % (name, c['Hk'], c['Wk'], d, mname, tk[0], tk[1], tk[2], tc[0], tc[1], tc[2], native.gen_attn_route(d, HEADS, 1, 1, c['Hk'], c['Wk'], dt)))
            js['%s %s one-row kernel us' % (name, mname)], js['%s %s one-row composite us' % (name, mname)] = tk[0], tc[0]
            del c


def window_report(args, lines, js):
    from hvrnet_amd.graphs import GraphedClip
    T, HW, PAD = FRAMES, (600, 1000), (608, 1008)
    GA = dict(spatial_range=-1, num_heads=HEADS, attention_type='1111', kv_stride=STRIDE)
    metas = [S.synth_meta(HW, PAD) for _ in range(T)]
    clip = torch.cat([S.synth_frame(i, img_hw=HW, pad_hw=PAD) for i in range(T)], 0).to(DEV)
    graphs = {}
    for which, swa in (('R-101', None), ('R-101 + attention in layer 3', ((), (), tuple(range(23)))), ('R-101 + attention in layers 2-3', ((), tuple(range(4)), tuple(range(23))))):
        cfg = hvr_config(frame_interval=T // 2, nms_post=300)
        sd = S.synth_state_dict('hvr')
        if swa is not None:
            cfg.model.backbone = dict(cfg.model.backbone, gen_attention=GA, stage_with_gen_attention=swa)
            sd = S.synth_state_dict('hvr', gen_attention=GA, stage_with_gen_attention=swa)
        model = hvrnet_amd.build_model(cfg, sd, torch.bfloat16, DEV)
        graphs[which] = GraphedClip(model, clip, metas, rescale=True)
    lines.append('')
    lines.append('one clip window (T = 15, 608 x 1008, 300 proposals, bf16, HVR head), hipGraph replay, ms per window (median of %d),' % args.windows)
    lines.append('the three models alternating %d times (23 attention blocks in layer 3, 4 in layer 2; their stages run at full resolution):' % args.reps)
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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--group', type=int, default=20, help='launches between two events (fewer for slow calls: a group is 5 ms at most)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--torch-cap', type=float, default=24e9, help="bytes the 'torch' yardstick may hold (it is run on fewer frames and scaled to fit)")
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('gen_attention_bench needs the GPU: nothing here can be measured without one')
    lines, js = Report(), {}
    lines.append('tools/gen_attention_bench.py on %s' % torch.cuda.get_device_name(0))
    core_report(args, lines, js)
    lines.append('split half: the block casts its map to f32, runs the f32 row above and casts back (two casts of the map, not timed here)')
    one_row_report(args, lines, js)
    if not args.no_window:
        window_report(args, lines, js)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
