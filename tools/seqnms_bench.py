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

Several problems per launch and tube outputs (native.seq_nms_batched); with --problems or --against only these run:

  --problems P [P ...]   P independent videos of that size side by side in ONE call against P single calls in sequence, and the
                         single call's time for scale; the two versions alternate --reps times, every figure is listed.  The
                         batched result must equal the single calls' bit for bit.
  --frames F [F ...]     the video lengths of these reports (default 60 300).
  --tubes                also time the same batched call with tube outputs, and record the table size.
  --against LIB          time hvr_seq_nms (and two calls in sequence) of THIS build against another build of the library, e.g. one
                         built from the parent commit, through the same buffers, alternating --reps times.

    python tools/seqnms_bench.py --problems 1 2 --tubes --against other/libhvr_hip.so --out profiles/seqnms_tubes.txt

Prints a text report (and one JSON line last); --out also writes the report to a file.
"""
import argparse
import ctypes
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


def videos(P, Fn):
    """P seeded videos of Fn frames (video 0 is video_report's) stacked -> device boxes [P*Fn,300,4], scores [P*Fn,300,31]"""
    vs = [R.video(9000 + Fn + 17 * p, Fn, 300, 31, tracks=8, clutter=0.5) for p in range(P)]
    return torch.as_tensor(np.concatenate([v[0] for v in vs])).to(DEV), torch.as_tensor(np.concatenate([v[1] for v in vs])).to(DEV)


def alternate(fns, reps, iters):
    """fns: [(name, fn)] timed in turn, `reps` rounds -> {name: [median us of each round]}"""
    out = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            out[name].append(timed(fn, 2, iters)[0])
            print('  .. %s: %.2f ms' % (name, out[name][-1] / 1e3), file=sys.stderr, flush=True)   # (progress; the report comes last)
    return out


def span(us):
    return '%.2f ms (rounds: %s)' % (statistics.median(us) / 1e3, ', '.join('%.2f' % (u / 1e3) for u in us))


def result_buffers(Ftot, max_tubes=None, P=1):
    out = (torch.empty((Ftot, ARGS[3], 5), device=DEV), torch.empty((Ftot, ARGS[3]), dtype=torch.long, device=DEV),
           torch.empty(Ftot, dtype=torch.int32, device=DEV))
    if max_tubes is not None:
        out += (torch.empty((Ftot, ARGS[3]), dtype=torch.int32, device=DEV), torch.empty((max_tubes, 4), dtype=torch.int32, device=DEV),
                torch.empty(max_tubes, device=DEV), torch.empty(P + 1, dtype=torch.int32, device=DEV))
    return out


def batched_report(P, Fn, iters, reps, tubes, lines, js):
    b, s = videos(P, Fn)
    counts = [Fn] * P
    singles = [result_buffers(Fn) for _ in range(P)]
    bat = result_buffers(P * Fn)

    def in_sequence():
        for p in range(P):
            native.seq_nms(b[p * Fn:(p + 1) * Fn], s[p * Fn:(p + 1) * Fn], *ARGS, out=singles[p])

    fns = [('one single call', lambda: native.seq_nms(b[:Fn], s[:Fn], *ARGS, out=singles[0])),
           ('%d single calls in sequence' % P, in_sequence),
           ('one batched call, P = %d' % P, lambda: native.seq_nms_batched(b, s, counts, *ARGS, out=bat))]
    if tubes:
        max_tubes = 30 * P * Fn * 300
        tub = result_buffers(P * Fn, max_tubes, P)
        fns.append(('one batched call, P = %d, tubes' % P, lambda: native.seq_nms_batched(b, s, counts, *ARGS, tubes=True, max_tubes=max_tubes, out=tub)))
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(bat[k][p * Fn:(p + 1) * Fn], singles[p][k]) for p in range(P) for k in range(3))
    same = same and (not tubes or all(torch.equal(x, y) for x, y in zip(bat, tub[:3])))
    t = alternate(fns, reps, iters)
    lines.append('P = %d videos of F = %d frames (R = 300, 31 classes; %d path workgroups): batched == single calls bit for bit: %s' % (P, Fn, 30 * P, same))
    for name, _ in fns:
        lines.append('  %-38s %s' % (name, span(t[name])))
        js['P=%d F=%d / %s us' % (P, Fn, name)] = t[name]
    seq, one = statistics.median(t[fns[1][0]]), statistics.median(t[fns[2][0]])
    lines.append('  batched / in sequence = %.3f (1/P = %.3f);  batched / one single call = %.2f' % (one / seq, 1.0 / P, one / statistics.median(t[fns[0][0]])))
    js['P=%d F=%d / ratio' % (P, Fn)] = one / seq
    if tubes:
        total = int(tub[6][-1].item())
        tb = statistics.median(t[fns[3][0]])
        lines.append('  tubes / no tubes = %.4f;  %d tubes (%d longer than one box): table %d bytes written of %d allocated (the candidate bound), ids %d bytes' % (
            tb / one, total, int((tub[4][:total, 3] > 1).sum().item()), total * 20, max_tubes * 20, P * Fn * ARGS[3] * 4))
        js['P=%d F=%d / tubes ratio' % (P, Fn)], js['P=%d F=%d / tubes' % (P, Fn)] = tb / one, total
    assert same, 'the batched call differs from the single calls'


def against_report(path, frames, iters, reps, lines, js):
    """hvr_seq_nms of this build and of the library at `path` (same signature) on the same device buffers, alternating."""
    other = ctypes.CDLL(os.path.abspath(path))
    for name in ('hvr_seq_nms', 'hvr_seq_nms_workspace_bytes'):
        getattr(other, name).restype, getattr(other, name).argtypes = native.SYMBOLS[name]
    lines.append('against %s sha256 %s (hvr_seq_nms through ctypes on both builds, the same buffers)' % (
        os.path.basename(path), hashlib.sha256(open(path, 'rb').read()).hexdigest()[:16]))
    for Fn in frames:
        b, s = videos(2, Fn)
        outs = {}
        ws = torch.empty(int(max(native.lib().hvr_seq_nms_workspace_bytes(Fn, 300, 31), other.hvr_seq_nms_workspace_bytes(Fn, 300, 31))),
                         dtype=torch.uint8, device=DEV)

        def call(lib, tag, p):
            out = outs.setdefault((tag, p), result_buffers(Fn))
            rc = lib.hvr_seq_nms(native._ptr(b[p * Fn:(p + 1) * Fn]), native._ptr(s[p * Fn:(p + 1) * Fn]), Fn, 300, 31, ARGS[0], ARGS[1], ARGS[2], 1, ARGS[3],
                                 native._ptr(out[0]), native._ptr(out[1]), native._ptr(out[2]), native._ptr(ws), ws.numel(), native._stream())
            assert rc == 0, (tag, rc)

        fns = [('this build, one call', lambda: call(native.lib(), 'new', 0)), ('other build, one call', lambda: call(other, 'old', 0)),
               ('this build, two calls in sequence', lambda: (call(native.lib(), 'new', 0), call(native.lib(), 'new', 1))),
               ('other build, two calls in sequence', lambda: (call(other, 'old', 0), call(other, 'old', 1)))]
        for _, fn in fns:
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for p in range(2) for x, y in zip(outs[('new', p)], outs[('old', p)]))
        t = alternate(fns, reps, iters)
        lines.append('F = %d: the two builds\' outputs are equal bit for bit: %s' % (Fn, same))
        for name, _ in fns:
            lines.append('  %-38s %s' % (name, span(t[name])))
            js['against F=%d / %s us' % (Fn, name)] = t[name]
        new, old = t[fns[0][0]], t[fns[1][0]]
        lines.append('  this / other = %.4f;  other build\'s spread over the rounds %.2f %%, this build\'s %.2f %%' % (
            statistics.median(new) / statistics.median(old), 100 * (max(old) - min(old)) / statistics.median(old), 100 * (max(new) - min(new)) / statistics.median(new)))
        assert same, 'the two builds disagree'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--problems', type=int, nargs='+', default=None)
    ap.add_argument('--frames', type=int, nargs='+', default=[60, 300])
    ap.add_argument('--tubes', action='store_true')
    ap.add_argument('--against', default=None)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    iters = max(10, args.iters)
    lines, js = [], {}
    so = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), 'libhvr_hip.so')
    lines.append('libhvr_hip.so sha256 %s' % hashlib.sha256(open(so, 'rb').read()).hexdigest()[:16])
    lines.append('seq_nms(score_thr %g, link_iou_thr %g, nms_iou_thr %g, max_num %d, rescore %r); HIP events, median of %d after warm-up' % (ARGS + (iters,)))
    if args.problems or args.against:
        lines.append('every figure: the median of the %d per-round medians, the rounds alternating between the versions' % args.reps)
        if args.against:
            against_report(args.against, args.frames, iters, args.reps, lines, js)
        for P in args.problems or []:
            for Fn in args.frames:
                batched_report(P, Fn, iters, args.reps, args.tubes, lines, js)
        text = '\n'.join(lines)
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text + '\n')
        print(json.dumps(js))
        return
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
