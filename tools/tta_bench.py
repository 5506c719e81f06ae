"""Cost of multi-scale / flip test-time augmentation per window (HIP events, one process): T = 15 frames, 600 x 1000 (padded
608 x 1008) plus a second scale 480 x 800, 300 proposals, HVR head, bf16 and split half (f16x2).

  t_plain(scale) = one eager `forward_feat` window on that scale's C4 maps (the un-augmented path)
  t_aug(2)       = one `forward_feat_aug` window on the flip pair of the first scale       vs 2 x t_plain(scale 1)
  t_aug(4)       = one `forward_feat_aug` window on two scales x flip                      vs 2 x t_plain(scale 1) + 2 x t_plain(scale 2)

The C4 maps are computed once before the timed loops (the backbone runs per frame, outside a window).  Prints one JSON line.
`--trace-only N`: run N augmented windows (A = 4, bf16) and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/tta_bench.py --trace-only 20`.
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
T, N = 15, 300
SCALES = [((600, 1000), (608, 1008), 1.0), ((480, 800), (480, 800), 0.8)]


def build_inputs(model):
    """-> per (scale, flip) augmentation: (list of T C4 maps, list of T metas), scale outer, flip inner."""
    augs = []
    for img_hw, pad_hw, s in SCALES:
        for flip in (False, True):
            metas = [dict(ori_shape=(600, 1000, 3), img_shape=img_hw + (3,), pad_shape=pad_hw + (3,), scale_factor=s, flip=flip) for _ in range(T)]
            c4 = []
            for i in range(T):
                im = S.synth_frame(i, img_hw=img_hw, pad_hw=pad_hw)
                if flip:
                    im = im.clone()
                    im[:, :, :img_hw[0], :img_hw[1]] = torch.flip(im[:, :, :img_hw[0], :img_hw[1]], dims=[3])
                c4.append(model(img=im.to(DEV), img_meta=[metas[i]], backbone_feat=True)[0])
            augs.append((c4, metas))
    return augs


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def nested(augs, which):
    x = [[augs[a][0][t] for a in which] for t in range(T)]
    metas = [[augs[a][1][t] for a in which] for t in range(T)]
    return x, metas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace-only', type=int, default=0)
    args = ap.parse_args()
    sd = S.synth_state_dict('hvr')
    out = dict(T=T, proposals=N, scales=[list(s[0]) for s in SCALES], iters=args.iters)
    modes = [('bf16', torch.bfloat16)] if args.trace_only else [('bf16', torch.bfloat16), ('f16x2', native.SPLIT)]
    for name, dtype in modes:
        model = hvrnet_amd.build_model(hvr_config(frame_interval=T // 2, nms_post=N), sd, dtype, DEV)
        with torch.no_grad():
            augs = build_inputs(model)
            x2, m2 = nested(augs, [0, 1])
            x4, m4 = nested(augs, [0, 1, 2, 3])
            if args.trace_only:
                for _ in range(args.trace_only):
                    model.forward_feat_aug(x4, m4, rescale=True)
                torch.cuda.synchronize()
                print(json.dumps(dict(trace_only=args.trace_only, mode=name)))
                return
            plain = [timed(lambda a=a: model.forward_feat(augs[a][0], augs[a][1], rescale=True), args.warmup, args.iters) for a in (0, 2)]
            aug2 = timed(lambda: model.forward_feat_aug(x2, m2, rescale=True), args.warmup, args.iters)
            aug4 = timed(lambda: model.forward_feat_aug(x4, m4, rescale=True), args.warmup, args.iters)
            pend = model.forward_feat_aug(x4, m4, rescale=True, defer=True)
            pend.result()
        sum2, sum4 = 2 * plain[0], 2 * plain[0] + 2 * plain[1]
        out[name] = dict(t_plain_ms=[round(v, 3) for v in plain], t_aug2_ms=round(aug2, 3), t_aug4_ms=round(aug4, 3),
                         sum_plain2_ms=round(sum2, 3), sum_plain4_ms=round(sum4, 3), ratio2=round(aug2 / sum2, 3), ratio4=round(aug4 / sum4, 3),
                         respeculated=bool(pend.respeculated))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
