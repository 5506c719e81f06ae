"""Cost of the Seq-NMS read-out of a whole video (hvrnet_amd.seq_nms, csrc/seqnms.hip) on a seeded synthetic video -- tracks plus
clutter (tests/seqnms_refs.py: video), R = 300 rows, 31 classes, F = 60 and F = 300 frames -- in one process on an otherwise idle chip:

  kernels  HIP-event times of the link / overlap kernel, the per-class path kernel and the per-frame merge, each alone
           (hvr_seq_nms_phases on the workspace the earlier phases filled), and of the whole call; warm-up, median of --iters runs.
  paths    the selected-path counts of the video: total, and how many are longer than one box -- exact for one class at F = 60 (the
           host restatement counts its rounds), and for all classes counted on the device's output as runs of one rescored score
           over consecutive frames.
  host     the numpy restatement (tests/seqnms_refs.py: seq_nms_ref, the plain loop) on class 1 of the F = 60 video, wall clock,
           once (it takes minutes per class); its output must equal the device's on the same input bit for bit.
  window   the per-window time of the plain greedy loop (forward_feat(defer=True) + result() on a full-size clip's C4 maps, T = 15,
           608 x 1008, 300 proposals, bf16 HVR head, both branches) -- the code the parent commit has, unchanged here -- so that
           F x window can be set against the post-processing.  --no-window skips it.

    python tools/seqnms_bench.py [--iters 20] [--out profiles/seqnms_video.txt]

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvrnet_amd  # noqa: E402
from hvrnet_amd import native, synthetic as S  # noqa: E402
from hvrnet_amd.config import hvr_config  # noqa: E402
from tests import seqnms_refs as R  # noqa: E402

DEV = 'cuda:0'
ARGS = (0.001, 0.5, 0.3, 300, 'avg')     # score_thr, link_iou_thr, nms_iou_thr, max_num, rescore: the configs' read-out + the defaults
ALL_ROWS = 30 * 300                      # max_num of the calls whose output the paths are counted on: no kept box is cut away


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


def video_report(Fn, iters, lines, js, host):
    boxes, scores = R.video(9000 + Fn, Fn, 300, 31, tracks=8, clutter=0.5)
    b, s = torch.as_tensor(boxes).to(DEV), torch.as_tensor(scores).to(DEV)
    cand = int((scores[:, :, 1:] > ARGS[0]).sum())
    out = native.seq_nms(b, s, *ARGS)
    torch.cuda.synchronize()
    kept = int(out[2].sum().item())
    lines.append('F = %d frames, R = 300, 31 classes: %d candidates (score > %g), %d boxes in the output (max_num 300 per frame)' % (Fn, cand, ARGS[0], kept))
    for name, mask in (('link / overlap kernel', 1), ('path kernel (30 workgroups)', 2), ('merge kernel', 4), ('whole call', None)):
        # (iters of the long kernels are capped: a run is tens of milliseconds)
        t = timed(lambda: native.seq_nms(b, s, *ARGS, phases=mask, out=out), 3, iters if mask != 2 and mask is not None else max(5, iters // 2))
        lines.append('  %-30s %10.1f us  (min %.1f, max %.1f)' % ((name,) + t))
        js['F=%d / %s us' % (Fn, name)] = t[0]
    again = native.seq_nms(b, s, *ARGS)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, again)), 'the phase-wise runs changed the result'
    # paths counted on the device's output: a maximal run of consecutive frames that hold a kept box of one class with one rescored
    # score ('avg': every box of a path carries the path's score; two paths of one class share a score only by coincidence)
    d, l, n = [t.cpu().numpy() for t in native.seq_nms(b, s, *ARGS[:3], ALL_ROWS, ARGS[4])]

    def runs(cls):
        paths = longp = 0
        for c in cls:
            seen = {}
            for t in range(Fn):
                for sc in d[t, :n[t]][l[t, :n[t]] == c][:, 4]:
                    seen.setdefault(sc.tobytes(), []).append(t)
            for ts in seen.values():
                ts = sorted(set(ts))
                starts = [t for i, t in enumerate(ts) if i == 0 or ts[i - 1] != t - 1]
                ends = [t for i, t in enumerate(ts) if i + 1 == len(ts) or ts[i + 1] != t + 1]
                paths += len(starts)
                longp += sum(e > s0 for s0, e in zip(starts, ends))
        return paths, longp

    allp = runs(range(30))
    lines.append('  %d boxes kept before the max_num cut; selected paths, all 30 classes (score runs of the device output): %d, longer than one box: %d' % (
        (int(n.sum()),) + allp))
    js['F=%d / paths' % Fn], js['F=%d / long paths' % Fn] = allp
    if host:
        # the host restatement on ONE class (the plain loop takes minutes per class at this size), against the device on the same input
        s1 = np.ascontiguousarray(scores[:, :, :2])
        s1d = torch.as_tensor(s1).to(DEV)            # uploaded once: the timed calls below hold no copy
        dev1 = [t.cpu().numpy() for t in native.seq_nms(b, s1d, *ARGS[:3], 300, ARGS[4])]
        info = {}
        t0 = time.time()
        want = R.seq_nms_ref(boxes, s1, *ARGS[:3], 300, ARGS[4], info=info)
        dt = time.time() - t0
        same = all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
                   for x, y in zip(dev1, want))
        one = timed(lambda: native.seq_nms(b, s1d, *ARGS), 2, 5)
        lines.append('  class 1 alone: host restatement (numpy, plain loop, once) %.1f s;  device %.1f us;  device == host bit for bit: %s' % (dt, one[0], same))
        lines.append('  class 1 alone: %d candidates, selected paths (exact, host): %d, longer than one box: %d;  %.2f us of the device call per path' % (
            int((s1[:, :, 1] > ARGS[0]).sum()), info['paths'], info['long_paths'], one[0] / max(info['paths'], 1)))
        js['F=%d / class 1 host s' % Fn], js['F=%d / class 1 device us' % Fn] = dt, one[0]
        js['F=%d / class 1 paths' % Fn], js['F=%d / class 1 long paths' % Fn], js['F=%d / class 1 equal' % Fn] = info['paths'], info['long_paths'], same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    iters = max(10, args.iters)
    lines, js = [], {}
    so = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), 'libhvr_hip.so')
    lines.append('libhvr_hip.so sha256 %s' % hashlib.sha256(open(so, 'rb').read()).hexdigest()[:16])
    lines.append('seq_nms(score_thr %g, link_iou_thr %g, nms_iou_thr %g, max_num %d, rescore %r); HIP events, median of %d after warm-up' % (ARGS + (iters,)))
    video_report(60, iters, lines, js, host=not args.no_host)
    video_report(300, iters, lines, js, host=False)
    if not args.no_window:
        T, N = 15, 300
        model = hvrnet_amd.build_model(hvr_config(frame_interval=T // 2, nms_post=N), S.synth_state_dict('hvr'), torch.bfloat16, DEV)
        metas = [S.synth_meta() for _ in range(T)]
        clip = torch.cat([S.synth_frame(i) for i in range(T)], 0).to(DEV)
        with torch.no_grad():
            c4 = model(img=clip, img_meta=metas, backbone_feat=True)[0]
            w = timed(lambda: model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True, defer=True).result(), 5, iters)
            r = timed(lambda: model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True, raw=True), 5, iters)
        lines.append('one full-size window of the plain greedy loop (T = 15, 608 x 1008, 300 proposals, bf16, both branches, from C4 maps): '
                     '%.3f ms (min %.3f, max %.3f); read out raw (no per-frame NMS): %.3f ms' % (w[0] / 1e3, w[1] / 1e3, w[2] / 1e3, r[0] / 1e3))
        lines.append('  (measured with THIS build, not with a build of the parent commit: the greedy window path is the same code in both; the parent\'s own '
                     'record of this window is 2.771 ms, profiles/softnms_readout.txt)')
        js['window ms'], js['window raw ms'] = w[0] / 1e3, r[0] / 1e3
        for Fn in (60, 300):
            whole = js['F=%d / whole call us' % Fn] / 1e3
            lines.append('  F = %3d: %d windows %.1f ms; Seq-NMS per branch %.2f ms = %.1f %% of them (two branches: x2)' % (
                Fn, Fn, Fn * w[0] / 1e3, whole, 100 * whole / (Fn * w[0] / 1e3)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(js))


if __name__ == '__main__':
    main()
