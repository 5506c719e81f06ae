"""Cost of the Soft-NMS read-out (test_cfg.rcnn.nms type='soft_nms') against the greedy read-out of the same build, in one process on
an otherwise idle chip (HIP events, warm-up, median of --iters >= 20 runs):

  chain    one branch's read-out chain -- decode (softmax + delta2bbox) + class kernel + merge -- on the decoded logits of the
           benchmark clip (synthetic clip 0, T = 15, 608 x 1008, 300 proposals, bf16 HVR head, branch 0), and the class kernel + merge
           alone on a clustered 300-box list with softmax-like scores; linear and gaussian against greedy.  Reports candidates,
           survivors (= rounds) per class and us per round: the Soft-NMS launch pair's time over the largest class's rounds, an
           upper bound of the round cost because the merge is inside.  Then four such read-outs as ONE launch pair (P = 4) against
           four launch pairs: what a call with several clips gains by handing a branch's read-outs over together.
  window   one full-size window, eager (`forward_feat(defer=True)` + result on the clip's C4 maps: the window without its backbone)
           and replayed from a hipGraph holding 4 clips (GraphedClip(windows=4): backbone included, ms per clip; a branch's four Soft-NMS
           read-outs go to one launch pair there), type='soft_nms'
           against type='nms': the difference is the feature's cost per window.

    python tools/softnms_bench.py [--iters 30] [--out profiles/softnms_readout.txt]

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
from hvrnet_amd.graphs import GraphedClip  # noqa: E402
from tests import softnms_refs as R  # noqa: E402

DEV = 'cuda:0'
T, N = 15, 300
CFGS = [('greedy', dict(type='nms', iou_thr=0.3)),
        ('soft linear', dict(type='soft_nms', iou_thr=0.5, min_score=0.05)),
        ('soft gaussian', dict(type='soft_nms', iou_thr=0.5, method='gaussian', sigma=0.5, min_score=0.05)),
        ('soft linear, defaults', dict(type='soft_nms', iou_thr=0.3)),
        ('soft gaussian, min_score 1e-3', dict(type='soft_nms', iou_thr=0.3, method='gaussian', sigma=0.5, min_score=1e-3))]


def timed(fn, warmup, iters):
    """-> (median, min, max) in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    return statistics.median(us), min(us), max(us)


def clustered(seed, n, ncls=31):
    """The clustered list of the tests (tests/softnms_refs.py): boxes [n,4] and softmax-like scores [n,ncls] on the device."""
    return torch.as_tensor(R.clustered_dets(seed, n)[:, :4]).to(DEV), torch.as_tensor(R.class_scores(seed + 1, n, ncls)).to(DEV)


def per_class(boxes, scores, cfg, thr=0.001):
    """-> (candidates [nfg], survivors [nfg]) of a read-out; survivors of a Soft-NMS class = its rounds."""
    nfg = scores.shape[1] - 1
    cand = (scores[:, 1:] > thr).sum(0).cpu().numpy()
    dets, labels, n = native.readout_nms(boxes, scores, thr, cfg, max(boxes.shape[0] * nfg, 1))
    k = int(n.item())
    return cand, np.bincount(labels[:k].cpu().numpy(), minlength=nfg)


def chain_report(name, boxes, scores, decode, iters, lines, js):
    lines.append('%s: R = %d rows, %d foreground classes, score_thr 0.001, max_per_img 300' % (name, boxes.shape[0], scores.shape[1] - 1))
    if decode is not None:
        t = timed(decode, 10, iters)
        lines.append('  decode alone                         %8.1f us  (min %.1f, max %.1f)' % t)
        js[name + ' / decode'] = t[0]
    base = None
    for cname, cfg in CFGS:
        cand, surv = per_class(boxes, scores, cfg)
        nms = timed(lambda: native.readout_nms(boxes, scores, 0.001, cfg, 300), 10, iters)
        row = '  %-30s nms %8.1f us (min %.1f, max %.1f)' % ((cname,) + nms)
        if decode is not None:
            full = timed(lambda: native.readout_nms(*reversed(decode()), 0.001, cfg, 300), 10, iters)
            row += '   decode + nms %8.1f us' % full[0]
            js['%s / %s / chain' % (name, cname)] = full[0]
        js['%s / %s / nms' % (name, cname)] = nms[0]
        if cname == 'greedy':
            base = nms[0]
        else:
            rounds = int(surv.max())
            row += '   x%.2f of greedy;  rounds per class min / median / max %d / %d / %d, <= %.2f us per round' % (
                nms[0] / base, surv.min(), int(np.median(surv)), rounds, nms[0] / max(rounds, 1))
        lines.append(row)
        lines.append('      candidates per class min / median / max %d / %d / %d;  survivors per class %d / %d / %d (total %d)' % (
            cand.min(), int(np.median(cand)), cand.max(), surv.min(), int(np.median(surv)), surv.max(), surv.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-window', action='store_true')
    args = ap.parse_args()
    iters = max(20, args.iters)
    lines, js = [], {}
    model = hvrnet_amd.build_model(hvr_config(frame_interval=T // 2, nms_post=N), S.synth_state_dict('hvr'), torch.bfloat16, DEV)
    metas = [S.synth_meta() for _ in range(T)]
    clips = [torch.cat([S.synth_frame(100 * c + i) for i in range(T)], 0).to(DEV) for c in range(4)]
    head = model.bbox_head
    with torch.no_grad():
        c4 = model(img=clips[0], img_meta=metas, backbone_feat=True)[0]
        # ---- the benchmark clip's decode arguments (branch 0) ----
        captured = []
        real = type(head)._decode

        def rec(*a):
            captured.append(a)
            return real(head, *a)

        head._decode = rec
        model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
        del head._decode
        dec_args = captured[0]
        scores, boxes = real(head, *dec_args)
        chain_report('benchmark clip, branch 0', boxes, scores, lambda: real(head, *dec_args), iters, lines, js)
        cb, cs = clustered(13100, 300)
        chain_report('clustered 300-box list', cb, cs, None, iters, lines, js)
        # ---- P = 4 problems in one launch pair against four launch pairs (what a 4-clip call's branch hands over) ----
        lines.append('four read-outs of the benchmark clip\'s branch: one launch pair with P = 4 against four launch pairs with P = 1')
        b4, s4 = torch.stack([boxes] * 4), torch.stack([scores] * 4)
        for cname, cfg in CFGS[1:3]:
            kw = dict(method=cfg.get('method', 'linear'), sigma=cfg.get('sigma', 0.5), min_score=cfg['min_score'])
            one = timed(lambda: native.multiclass_soft_nms(b4, s4, 0.001, cfg['iou_thr'], 300, **kw), 10, iters)
            four = timed(lambda: [native.multiclass_soft_nms(boxes, scores, 0.001, cfg['iou_thr'], 300, **kw) for _ in range(4)], 10, iters)
            lines.append('  %-16s P = 4: %8.1f us (min %.1f, max %.1f)   4 x P = 1: %8.1f us (min %.1f, max %.1f)   x%.2f' % (
                (cname,) + one + four + (four[0] / one[0],)))
            js['batched / %s / P=4' % cname], js['batched / %s / 4 x P=1' % cname] = one[0], four[0]
        # ---- one full-size window ----
        if not args.no_window:
            lines.append('one full-size window (T = 15, 608 x 1008, 300 proposals, bf16, both branches):')
            res = {}
            for cname, cfg in CFGS[:3]:
                model.test_cfg.rcnn.nms = dict(cfg)

                def eager():
                    model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True, defer=True).result()

                e = timed(eager, 5, iters)
                g = GraphedClip(model, torch.cat(clips, 0), metas * 4, rescale=True, n_out=1, windows=4)

                def replay():
                    for p in g.run():
                        p.result()

                r = timed(replay, 5, iters)
                res[cname] = (e[0] / 1e3, r[0] / 4e3)
                lines.append('  %-16s eager, from C4 maps %8.3f ms (min %.3f, max %.3f)   graph replay with backbone, 4 clips per graph %8.3f ms per clip (min %.3f, max %.3f)' % (
                    cname, e[0] / 1e3, e[1] / 1e3, e[2] / 1e3, r[0] / 4e3, r[1] / 4e3, r[2] / 4e3))
                js['window / %s / eager ms' % cname], js['window / %s / graph ms per clip' % cname] = e[0] / 1e3, r[0] / 4e3
                del g
            for cname in ('soft linear', 'soft gaussian'):
                lines.append('  %-16s - greedy: eager %+.3f ms (x%.3f), graph replay %+.3f ms per clip (x%.3f)' % (
                    cname, res[cname][0] - res['greedy'][0], res[cname][0] / res['greedy'][0], res[cname][1] - res['greedy'][1],
                    res[cname][1] / res['greedy'][1]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
