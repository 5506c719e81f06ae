"""Headline benchmark: VID key-frame detections / second, R101 Faster-RCNN + HVR (or SELSA) head,
1000x600 frames (padded 608x1008), 300 proposals / frame, T = 15 frames / window.

    python bench.py --gpus 1 --steps 20 --warmup 3                  # the headline region alone: the contract keys
    python bench.py --gpus 1 --steps 20 --warmup 3 --full           # + every other measurement and check below
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR   # + the last timed call's detections as DIR/*.npy
    python bench.py --gpus 2                      # launches the two ranks itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

One step = one window in CLIP MODE (BASELINE.json configs[2]): all T frames go through
backbone -> res5 -> RPN -> proposals -> RoIAlign -> relation head -> read-out, nothing cached between
steps, and one key-frame detection comes out (per-class arrays on the host, as the reference's
bbox2result returns them).  Frames are already resident in HBM when timing starts.  Ranks run
independent clips (no data-path collective): weak scaling, value = N * steps / max-over-ranks time.

Two timed regions of the same K steps, each bracketed by barrier + synchronize: (1) the eager single-lane loop -- the
region the `roofline` HIP events are taken in (a kernel's own duration: one window on the chip) and reported as
`single_lane`; (2) the HEADLINE region: the same windows replayed from hipGraphs on `--lanes` (4) HIP streams in turn, so
that four independent clips are in flight (measured, profiles/r04_lanes.txt: 2 lanes 162.7-165.5 frames/s, 4 lanes 171.5-174.4,
6 / 8 the same as 4, odd counts no better than 2 -- the lanes' streams share the runtime's four hardware queues) -- one
window's latency-bound phases (proposals, read-out, the relation stages'
one-round kernels' prologues and epilogues) run beside the other's dense phases, one host call per window.  Every window of
both regions is computed in full and its results are read on the host inside the region; the replayed windows' detections
are identical to the eager ones (tests/test_graphs_gpu.py).  `--lanes 1 --no-graphs` makes region (1) the headline.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment launches the N ranks itself (one process per
GPU under torch.distributed.run, 127.0.0.1 rendezvous -- what tools/dist_test.sh:9-10 does for the reference) and refuses
loudly when fewer than N devices are visible.

A plain run (no --full) sets up, warms up, times the headline region once (`--repeats`, default 1) and prints the contract keys
(`metric`, `value`, `unit`, `n_gpus`, `steps`, `warmup`, `ms_per_step`, `higher_is_better`, `dtype`, `config`, `value_spread`,
`per_rank`, `device`, `lib_sha16`); --full runs the headline region 5 times and everything below as well.

JSON line (one line, numbers only; README.md "Reading the bench line" says what every key means).  With --full, after the contract keys:
`within_tolerance` -- the fastest compute mode whose detections meet north_star's tolerance against the CPU oracle on the same
frames (dtype, frames/s, its relation-core roofline, its parity); `single_lane` -- the eager one-window-in-flight figure with its
own spread (the figure to compare builds with); `roofline` (relation core, HIP events inside the timed region); `cpu_baseline`
(the CPU oracle on whole windows: 1 warm-up + median of 3, plus configs[0]; rank 0, N = 1); `precision_ladder` (one compact row per
compute mode: eager / replayed throughput, roofline, parity, per-class kernel times); `kernel_classes` of the headline mode; side
loops (`ref_loop`, `cached_loop`, `graphed_clip`, `graphed_stream`, `train_step`); for N > 1 `per_rank`, `rccl_world_size` and
`train_allreduce` (the training step's one exchange: a flat f32 gradient buffer of the detector's trainable size).
"""
import argparse
import contextlib
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md; split half (f16x2) spends three half MFMAs per product, so the
# algorithmic flops it can deliver peak at a third of the half rate
MFMA_PEAK_TF = {'bf16': 2500.0, 'f16': 2500.0, 'f16x2': 2500.0 / 3.0, 'f32': 157.3}
MODE_WHAT = {
    'bf16': 'bf16 operands (v_mfma_f32_16x16x32_bf16), f32 accumulation / softmax / box arithmetic: the benchmark dtype BASELINE.json names',
    'f16': 'IEEE half operands (v_mfma_f32_16x16x32_f16) on the tile engine: the bf16 rate, 8 x finer mantissa',
    'f16x2': 'split half: every operand as hi + lo * 2^-11 halves (22 bits), three half MFMAs per product, f32 accumulation',
    'f32': 'f32 operands on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32, 1/16 of the half rate)'}
HBM_PEAK_GBS = 8000.0
# north_star's tolerance (class indices exact, scores within 1e-3, boxes within 1e-3 px + 1.3e-6 x the coordinate extent, the default f32 rtol
# of torch.testing): ONE definition, hvrnet_amd/parity.py, shared with tools/precision_ladder.py, the full-size tests and smoke()
from hvrnet_amd.parity import TOL_SCORE, TOL_BOX_PX, BOX_RTOL   # noqa: E402
XGMI_LINK_GBS, XGMI_LINKS = 153.0, 7           # per GPU, SURVEY.md section 5
# trainable f32 parameters whose gradients one training step exchanges (176 MB HVR / 271 MB SELSA)
TRAIN_GRAD_ELEMS = {'hvr': 44128768, 'selsa': 67700000}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--head', default='hvr', choices=['hvr', 'selsa'])
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f16', 'f16x2', 'f32'], help='compute mode of the headline region')
    ap.add_argument('--ladder', default='f16,f16x2,f32',
                    help='other compute modes timed after the headline (eager single lane with the relation launches tagged + the '
                         'headline\'s graph replay), each with its detections compared with the CPU oracle: the `precision_ladder` table')
    ap.add_argument('--full', action='store_true',
                    help='everything beside the headline: the eager single-lane and batched regions, `roofline`, the precision ladder, '
                         'the CPU oracle leg and the tolerance claim, per-class kernel times, side loops, hipGraph side legs, the training '
                         'step and (N > 1) the all-reduce.  Without it a run sets up, warms up, times the K steps and prints the contract keys')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write the detections of the last timed call (every clip of it) to DIR/*.npy (float32)')
    ap.add_argument('--repeats', type=int, default=None, help='the headline region (K steps) is timed this many times (default 1, with --full 5): '
                                                              'value = the median, `value_spread` lists all of them')
    ap.add_argument('--frames', type=int, default=15)
    ap.add_argument('--proposals', type=int, default=300)
    ap.add_argument('--tol-clips', type=int, default=8, help='synthetic clips the tolerance claim (`within_tolerance`) is checked on: the benchmark\'s + this many - 1 others')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='skip the CPU oracle leg (and with it the `parity` object)')
    ap.add_argument('--quick', action='store_true', help='cpu_baseline on a 3-frame sample (scaled) instead of whole windows')
    ap.add_argument('--no-f32-leg', action='store_true', help='skip the precision ladder (the other compute modes\' timings)')
    ap.add_argument('--no-train-step', action='store_true', help='skip the training-step side measurement (tools/train_bench.py)')
    ap.add_argument('--no-side-loops', action='store_true', help='skip ref_loop / cached_loop / two_in_flight (profiling runs)')
    ap.add_argument('--no-graphs', action='store_true', help='skip the hipGraph legs (graphed_clip / graphed_stream)')
    ap.add_argument('--inflight', type=int, default=int(os.environ.get('HVR_INFLIGHT', '1')),
                    help='independent windows enqueued on that many HIP streams in turn (throughput mode)')
    ap.add_argument('--clips', type=int, default=int(os.environ.get('HVR_CLIPS', '4')),
                    help='independent clips per call / per graph (round 5): every kernel up to the relation stages takes the W clips as '
                         'one batch, the relation core runs per clip in grouped launches (hvr_relation_fwd_grouped); a step stays ONE '
                         'window, a call is W steps (W is lowered to a divisor of --steps)')
    ap.add_argument('--lanes', type=int, default=int(os.environ.get('HVR_LANES', '0')),
                    help='headline region: windows replayed from hipGraphs on that many HIP streams in turn; 0 (default) = the divisor of steps / clips in 3..6 '
                         'that leaves no lane idle in the last round of replays (20 steps, 4 clips: 5 lanes), else 4 (1 with --no-graphs: the '
                         'eager single-lane loop is the headline, as in round 1)')
    ap.add_argument('--breakdown', action='store_true', help='print per-shape conv / gemm times of one window to stderr')
    ap.add_argument('--stub', action='store_true',
                    help='host-logic self-test of the launcher / barrier / max-over-ranks / JSON contract without a GPU: the window '
                         'is a fixed sleep and the process group is gloo (tests/test_bench_launcher.py); never a measurement')
    args = ap.parse_args(argv)
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    return args


def host_cores():
    """CPUs this process may actually use: min(affinity, cgroup quota). The GPU box shows 256 logical CPUs under a
    16-CPU cgroup quota; oversubscribing it makes the CPU path ~200x slower."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (IOError, OSError, ValueError):
        pass
    return max(1, n)


# ------------------------------------------------------------------------------------------ launcher
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args, argv):
    """`--gpus N` without a torchrun environment: start the N ranks (one process per GPU, tools/dist_test.sh:9-10) and
    return their exit code.  The children see WORLD_SIZE and run main() directly."""
    if not args.stub:
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            sys.stderr.write('bench.py: --gpus %d asked for but only %d GPU(s) are visible (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES?); '
                             'refusing to run fewer ranks than asked for\n' % (args.gpus, have))
            return 2
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')  # dmabuf IPC only on this driver: RCCL needs it across processes
    env.setdefault('OMP_NUM_THREADS', str(max(1, host_cores() // args.gpus)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------------------------------------ CPU oracle leg
def cpu_baseline_quick(head, T, n_prop, sd):
    """--quick: the oracle on 3 of the T frames (scaled by T/3) + the full-size relation head and read-out."""
    from hvrnet_amd import synthetic as S
    from oracle import hvr_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    ns = min(3, T)
    imgs = [S.synth_frame(i) for i in range(ns)]
    metas = [S.synth_meta() for _ in range(ns)]
    with torch.no_grad():
        O.resnet_c4(imgs[0][:, :, :128, :128], sd)  # warm-up of the thread pool / allocator
        t0 = time.time()
        c4 = [O.resnet_c4(im, sd) for im in imgs]
        x = torch.cat(c4, 0)
        c5 = O.shared_head(x, sd)
        cls, reg = O.rpn_forward(x, sd)
        base = O.gen_base_anchors(16, [4, 8, 16, 32], [0.5, 1.0, 2.0])
        anchors = O.grid_anchors(base, cls.shape[-2:], 16)
        cfg = dict(O.RPN_TEST_CFG, nms_post=n_prop, max_num=n_prop)
        props = [O.rpn_get_bboxes_single(cls[i], reg[i], anchors, metas[i]['img_shape'], cfg) for i in range(ns)]
        rois = [O.bbox2roi([p]) for p in props]
        torch.cat([O.roi_align(c5[i:i + 1], rois[i], 7, 1.0 / 16, 2) for i in range(ns)], 0)
        t_frames = time.time() - t0
        M = T * n_prop
        g = torch.Generator().manual_seed(0)
        roi_feats = torch.rand((M, 256, 7, 7), generator=g)
        cur = dict(start=(T // 2) * n_prop, length=n_prop)
        t0 = time.time()
        if head == 'hvr':
            cs, rs = O.hvr_head_forward_test(roi_feats, sd, cur, n_prop, T)
        else:
            c, r = O.selsa_head_forward(roi_feats, sd, cur, n_prop, T)
            cs, rs = [c], [r]
        key_rois = torch.cat([torch.zeros(n_prop, 1), torch.rand(n_prop, 4) * 500], 1)
        for c, r in zip(cs, rs):
            O.get_det_bboxes(key_rois, c, r, (600, 1000, 3), 1.0, True, O.RCNN_TEST_CFG)
        t_head = time.time() - t0
    window_s = t_frames * (T / float(ns)) + t_head
    return dict(value=round(1.0 / window_s, 4), unit='frames/s', cores=cores, kind='port',
                sample='--quick: %d of %d frames to RoIAlign (%.2f s, x%.1f) + full head M=%d (%.2f s)' % (ns, T, t_frames, T / float(ns), M, t_head),
                window_seconds=round(window_s, 3)), None


N64_CLIPS = 3   # clips whose oracle window is also evaluated in float64


def cpu_baseline_full(head, T, n_prop, sd, clip_ids):
    """SURVEY.md 8(d) "CPU baseline": the CPU oracle ("port": the PyTorch-CPU restatement oracle/hvr_oracle.py, pinned to the
    reference's modules by tests/golden), clip mode, whole windows on all usable host cores: configs[0] first (1 key + 2 reference
    frames, 32 proposals: the reference's own CPU-runnable case, and the warm-up), then ONE window of each clip in `clip_ids` (lists of
    synthetic frame ids; clip 0 is the benchmark's) -- the median of their times is the baseline, their results are the references the
    tolerance is checked against on every clip -- and the first N64_CLIPS clips once more in FLOAT64: how far the oracle's own f32 evaluation
    order moves its outputs (`oracle_noise_floor`).  -> (cpu_baseline dict, [one f32 result per clip], [one f64 result per clip], noise floor, [per clip the f32 run's per-frame proposal lists])."""
    from hvrnet_amd import parity, synthetic as S
    from oracle import hvr_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    metas = [S.synth_meta() for _ in range(T)]
    rpn_cfg = dict(O.RPN_TEST_CFG, nms_post=n_prop, max_num=n_prop)
    pick = (lambda r: r) if head == 'hvr' else (lambda r: r[0])
    times, wants, props = [], [], []
    with torch.no_grad():
        imgs0 = [S.synth_frame(i) for i in clip_ids[0]]
        t1 = []
        for it in range(3):
            t0 = time.time()
            O.clip_forward(imgs0[:3], metas[:3], sd, head, 1, 32, 3, rpn_cfg=dict(O.RPN_TEST_CFG, nms_post=32, max_num=32))
            t1.append(time.time() - t0)
        for ids in clip_ids:
            imgs = imgs0 if ids is clip_ids[0] else [S.synth_frame(i) for i in ids]
            t0 = time.time()
            r_, inter_ = O.clip_forward(imgs, metas, sd, head, T // 2, n_prop, T, rpn_cfg=rpn_cfg, return_intermediates=True)
            times.append(time.time() - t0)
            wants.append(pick(r_))
            props.append([p_.numpy() for p_ in inter_['proposals']])
        # the first N64 clips once more in FLOAT64 (22 s each on 16 cores): the reference the literal 1e-3 px reading is also printed against,
        # and the oracle's own f32-vs-f64 distance (tests/test_fullsize_gpu.py and tools/noise_budget.py print it for other clips / configs[1])
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        wants64, t64 = [], []
        for ids in clip_ids[:N64_CLIPS]:
            imgs = imgs0 if ids is clip_ids[0] else [S.synth_frame(i) for i in ids]
            t0 = time.time()
            wants64.append(pick(O.clip_forward([im.double() for im in imgs], metas, sd64, head, T // 2, n_prop, T, rpn_cfg=rpn_cfg)))
            t64.append(time.time() - t0)
    runs = sorted(times)
    window_s = runs[len(runs) // 2]
    c1 = sorted(t1[1:])[0]
    out = dict(value=round(1.0 / window_s, 4), unit='frames/s', cores=cores, kind='port',
               sample='whole %d-frame windows through oracle.clip_forward, one of each of %d synthetic clips after a configs[0] warm-up: median of (%s) s'
                      % (T, len(runs), ' / '.join('%.2f' % r for r in runs)),
               window_seconds=round(window_s, 3), config1_window_seconds=round(c1, 3))
    last = (lambda r: r[-1]) if head == 'hvr' else (lambda r: r)
    fl = [parity.strict(last(a), last(b)) for a, b in zip(wants, wants64)]
    floor = dict(class_flips=[f['class_flips'] for f in fl],   # oracle.clip_forward in float32 against the same code in float64, per clip
                 max_score_err=[float('%.3g' % f['max_score_err']) for f in fl], max_box_err=[float('%.3g' % f['max_box_err']) for f in fl],
                 f64_window_seconds=round(sorted(t64)[len(t64) // 2], 2))
    return out, wants, wants64, floor, props


def parity_object(head, dtype_name, got, want):
    """This run's detections against the CPU oracle's (oracle.clip_forward, f32, same frames and weights, final branch): position by
    position (class_flips, max_score_err, max_box_err in px) and, for results that keep different boxes at the discontinuous steps,
    box-to-box matching (`matched`: oracle detections with score >= 0.05 that reappear with the same class and IoU > 0.9)."""
    from hvrnet_amd import parity
    g, w = (got[-1], want[-1]) if head == 'hvr' else (got, want)
    st, tr = parity.strict(g, w), parity.track(g, w)
    return dict(dtype=dtype_name, class_flips=st['class_flips'], max_score_err=round(st['max_score_err'], 6), max_box_err=round(st['max_box_err'], 5),
                max_box_excess=round(st['max_box_excess'], 5), tie_swaps=st['tie_swaps'], detections=st['n'], matched=dict(n_ref=tr['n_ref'], same_class_frac=round(tr['same_class_frac'], 4),
                                                 max_score_err=round(tr['max_score_err'], 5), max_box_err=round(tr['max_box_err'], 4)))


def within_tolerance(pr):
    """north_star's bar on a parity object against the oracle's f32 evaluation (hvrnet_amd/parity.py: class indices exact, scores
    within TOL_SCORE, coordinates within TOL_BOX_PX + BOX_RTOL x extent)."""
    from hvrnet_amd import parity
    return parity.within_tolerance(pr)


def clip_distance(head, a, b):
    """How far two results of the SAME clip are apart (final branch, parity.strict position by position) -- e.g. clip 0 of a W-clip call
    (grouped relation core: one f32 sum associated differently, <= 1 output ulp of the operand format) against the one-window call.  In a
    mode that carries the tolerance the distance has to be inside it; in bf16 the discontinuous steps may amplify one ulp."""
    from hvrnet_amd import parity
    g, w = (a[-1], b[-1]) if head == 'hvr' else (a, b)
    st = parity.strict(g, w)
    return dict(identical=same_detections(a, b), class_flips=st['class_flips'], max_score_err=round(st['max_score_err'], 7), max_box_err=round(st['max_box_err'], 5),
                within_tolerance=parity.within_tolerance(st))


def same_detections(a, b):
    """Two results of the same window (per-class [k,5] arrays, one list per branch for the HVR head): every array equal bit for bit."""
    import numpy as np

    def flat(r):
        return [np.asarray(x) for br in (r if isinstance(r[0], (list, tuple)) else [r]) for x in br]
    fa, fb = flat(a), flat(b)
    return bool(len(fa) == len(fb) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(fa, fb)))


# Algorithmic flops of ONE training iteration (2 x multiply-adds of the dense products; SURVEY.md 8a's per-frame figures: stem 2.9, layer 1
# 16.3, layer 2 23.2, layer 3 124.6, res5 74.1, RPN 22.7 GF per 608 x 1008 frame; a trainable layer costs forward + dX + dW = 3 x):
#   selsa (1 key + 2 reference frames, frozen stem + layer 1): 3 frames x (19.2 + 3 x (147.8 + 74.1 + 22.7)) = 2.26 TF, + the head on
#          <= 3 x 256 sampled RoIs (fc_new_1 19.7 GF, fwd + bwd 0.06 TF) -> 2.3 TF
#   hvr   (5 videos x 3 frames, backbone + res5 + RPN without a graph on all 15, res5 with a graph on the 9 frames of the 3 chosen
#          videos): 15 x (167.0 + 74.1 + 22.7) + 9 x 3 x 74.1 = 5.96 TF, + the head 0.1 TF -> 6.1 TF
TRAIN_STEP_FLOPS = {'selsa': 2.3e12, 'hvr': 6.1e12}


def train_step_side_measurement(head):
    """configs[4] beside the headline, never as `value`: one training iteration of the same detector family (HNMBRCNN: 5 videos x 3
    frames in, 3 chosen; SelsaRCNN: 1 key + 2 reference frames) at 600x1000 / 300 proposals, bf16 operands with f32 master weights,
    measured by tools/train_bench.py in its own process after the timed region.  None if that run fails."""
    try:
        def run(extra):
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_bench.py'), '--head', head, '--steps', '10', '--warmup', '3'] + extra,
                               capture_output=True, text=True, timeout=300)
            return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        d = run([])
        ach = TRAIN_STEP_FLOPS[head] / (d['ms_per_step'] * 1e-3) / 1e12
        out = dict(iterations_per_s=d['value'], ms_per_iteration=d['ms_per_step'], input_frames_per_s=d['frames_per_s'], dtype=d['dtype'],
                   trainable_params=d['params'],
                   roofline=dict(bound='mfma', achieved=round(ach, 1), peak=MFMA_PEAK_TF['bf16'], unit='TFLOP/s', frac=round(ach / MFMA_PEAK_TF['bf16'], 4),
                                 flops_per_iteration=TRAIN_STEP_FLOPS[head]))   # whole iteration (forward, backward, targets, losses, clip + SGD) against the dense MFMA peak
        if d.get('backbone_prefetch'):
            # HVR: the frozen backbone of batch i + 1 runs on a second stream while batch i trains (dist_train.C4Prefetcher); the same
            # iteration with the backbone in line is reported beside it
            out['backbone_prefetch'] = True
            out['ms_per_iteration_backbone_in_line'] = run(['--no-prefetch'])['ms_per_step']
        return out
    except Exception as exc:   # noqa: BLE001 -- a side measurement must not take the headline down
        sys.stderr.write('train_step side measurement skipped: %r\n' % (exc,))
        return None


def allreduce_leg(dist, world, head, device, iters=5):
    """The training step's one exchange (mmdet/core/utils/dist_utils.py:9-28: one flat f32 all-reduce of every gradient)
    timed alone on a buffer of the detector's trainable size -- RCCL over xGMI on GPUs (gloo in --stub runs)."""
    n = TRAIN_GRAD_ELEMS[head]
    buf = torch.ones(n if device.type == 'cuda' else min(n, 1 << 20), dtype=torch.float32, device=device)
    nbytes = buf.numel() * 4

    def sync():
        if device.type == 'cuda':
            torch.cuda.synchronize(device)
    for _ in range(2):
        dist.all_reduce(buf)
    sync()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(buf)
    sync()
    ms = (time.perf_counter() - t0) / iters * 1e3
    t = torch.tensor([ms], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms = float(t.item())
    algbw = nbytes / (ms * 1e-3) / 1e9
    frac = 2.0 * (world - 1) / world
    return dict(bytes=nbytes,
                ms=round(ms, 4), algbw_gbs=round(algbw, 2), busbw_gbs=round(algbw * frac, 2),
                est_ring_one_link_ms=round(frac * nbytes / (XGMI_LINK_GBS * 1e9) * 1e3, 3),
                est_direct_all_links_ms=round(frac * nbytes / (min(world - 1, XGMI_LINKS) * XGMI_LINK_GBS * 1e9) * 1e3, 3),
                backend=dist.get_backend())


def stream_side_measurement(head):
    """The pipelined stream loop with two frames in flight (GraphedStream(frame_lanes=2)) and the window graph on a stream of its own
    (window_cus: the CUs of that stream; 256 = the chip), on 8 hardware queues, measured by tools/stream_bench.py in a process of its
    own: where a HIP stream's launches queue depends on how many streams the process has used before and on GPU_MAX_HW_QUEUES, which
    the runtime reads when it starts; after this script's ladder of graph builds the loop loses its gain (tools/stream_bench.py)."""
    def run(queues):
        env = dict(os.environ)
        env['GPU_MAX_HW_QUEUES'] = str(queues)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'stream_bench.py'), '--head', head], capture_output=True, text=True, timeout=300, env=env)
        return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    try:
        ss = run(8)
    except Exception as exc:   # noqa: BLE001 -- a side measurement must not take the headline down
        sys.stderr.write('stream side measurement skipped: %r\n' % (exc,))
        return None
    try:   # the same loop on the runtime's default of 4 hardware queues (what a caller gets who does not set the variable: INTEGRATION.md)
        d4 = run(4)
        ss['default_hw_queues'] = dict(hw_queues=d4.get('hw_queues', 4), window_on_confined_stream=d4.get('window_on_confined_stream'),
                                       window_on_the_callers_stream=d4.get('window_on_the_callers_stream'), ms_per_frame=d4.get('ms_per_frame'),
                                       same_detections=d4.get('same_detections'))
    except Exception as exc:   # noqa: BLE001
        sys.stderr.write('stream side measurement on the default queues skipped: %r\n' % (exc,))
    return ss


def synth_frames(ids):
    """[len(ids),3,608,1008] f32 on the host: synthetic.synth_frame of every id, on a few host threads (every frame has its own
    seeded generator, so the tensor is the same as one made frame by frame)."""
    from concurrent.futures import ThreadPoolExecutor
    from hvrnet_amd import synthetic as S
    with ThreadPoolExecutor(max(1, min(8, host_cores()))) as ex:
        return torch.cat(list(ex.map(S.synth_frame, ids)), 0)


def dump_outputs(path, clips, head):
    """--dump-outputs: the detections of the last timed call, one file per clip of it and branch of the head (HVR: every test
    branch; SELSA: one), DIR/clip<w>_branch<b>.npy, float32 [n, 6] = x1, y1, x2, y2, score, class index: the per-class [k, 5]
    arrays a caller receives, concatenated in class order."""
    os.makedirs(path, exist_ok=True)
    for w, r in enumerate(clips):
        branches = r if isinstance(r[0], (list, tuple)) else [r]
        for b, br in enumerate(branches):
            rows = [np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 5), np.full((len(a), 1), c, dtype=np.float32)], 1)
                    for c, a in enumerate(br)]
            np.save(os.path.join(path, 'clip%d_branch%d.npy' % (w, b)), np.concatenate(rows, 0) if rows else np.zeros((0, 6), np.float32))


def lib_sha16():
    from hvrnet_amd import native
    return hashlib.sha256(open(native.LIB_PATH, 'rb').read()).hexdigest()[:16]


def relation_traffic(units=1, dtype='bf16'):
    """HBM-side bytes per relation-core call (of `units` windows: the grouped call's PMC passes carry `groups`) from the committed PMC
    passes (bench.py cannot collect PMC itself): the newest profiles/r*_relation_traffic.json whose `lib_sha16` names THIS build of
    libhvr_hip.so and whose `groups` is `units`; None (stale) otherwise."""
    import glob
    sha = lib_sha16()
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_relation_traffic*.json')), reverse=True):
        try:
            d = json.load(open(path))
        except ValueError:
            continue
        if d.get('lib_sha16') == sha and int(d.get('groups', 1)) == int(units) and d.get('dtype', 'bf16') == dtype:
            return d.get('traffic_bytes_per_launch'), os.path.basename(path)
    return None, 'no profiles/r*_relation_traffic*.json was collected for this build (lib %s) with groups = %d, dtype %s: tools/collect_profiles.sh' % (sha, units, dtype)


# ------------------------------------------------------------------------------------------ stub (CPU host-logic self-test)
def stub_main(args, rank, local_rank, world):
    import torch.distributed as dist
    dev = torch.device('cpu')
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)

    def sync():
        if world > 1:
            dist.barrier()
    for _ in range(args.warmup):
        time.sleep(0.002)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))      # rank r is (1 + r)x slower: the reported time must be the slowest rank's
    sync()
    mine = time.perf_counter() - t0
    elapsed, per_rank, ar = mine, [mine], None
    if world > 1:
        t = torch.tensor([mine], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        allt = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allt, torch.tensor([mine], dtype=torch.float64))
        per_rank = [float(x.item()) for x in allt]
        if args.full:
            ar = allreduce_leg(dist, world, args.head, dev, iters=2)
    if rank == 0:
        out = dict(metric='STUB (launcher self-test, not a measurement)', value=round(world * args.steps / elapsed, 3), unit='frames/s',
                   n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=round(elapsed / args.steps * 1e3, 3),
                   higher_is_better=True, scaling='weak', vs_baseline=None, dtype='none', data='none',
                   config=dict(workload='stub'), per_rank=[dict(rank=i, frames_per_s=round(args.steps / t_, 3)) for i, t_ in enumerate(per_rank)],
                   rccl_world_size=(dist.get_world_size() if world > 1 else 1), gpus_requested=args.gpus)
        if ar is not None:
            out['train_allreduce'] = ar
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------ the benchmark
def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args, argv))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus:
        sys.stderr.write('bench.py: --gpus %d but the launcher started %d rank(s); the JSON line reports the ranks that ran\n' % (args.gpus, world))
    if args.stub:
        return stub_main(args, rank, local_rank, world)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if torch.cuda.device_count() <= local_rank:
            raise SystemExit('bench.py: rank %d has no GPU %d (%d visible)' % (rank, local_rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        dist.init_process_group('nccl', rank=rank, world_size=world)
    dev = torch.device('cuda', local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)

    import hvrnet_amd
    from hvrnet_amd import native, synthetic as S
    from hvrnet_amd.config import hvr_config, selsa_config

    T, n_prop = args.frames, args.proposals
    assert T % 2 == 1
    MODES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x2': native.SPLIT, 'f32': torch.float32}
    dt = MODES[args.dtype]
    cfg = (hvr_config if args.head == 'hvr' else selsa_config)(frame_interval=T // 2, nms_post=n_prop)
    sd = S.synth_state_dict(args.head)
    model = hvrnet_amd.build_model(cfg, sd, dt, dev)
    # each rank works on its own clip: different synthetic frames per rank
    frame_ids = [rank * 1000 + i for i in range(T)]
    frames = synth_frames(frame_ids).to(dev)  # [T,3,608,1008] resident in HBM
    metas = [S.synth_meta() for _ in range(T)]
    # W clips per call / per graph: a divisor of --steps (a step is one window); clip 0 of lane 0 is `frames`, every other clip of
    # every lane has frames of its own (lane k, clip w: ids rank * 1000 + 100 * (k * W + w) + i), so the graphs in flight read
    # lanes x W x 110 MB of distinct f32 input -- more than the 256 MB Infinity Cache holds
    W = max(1, args.clips)
    while args.steps % W:
        W -= 1

    def lane_frames(k):
        clips = [frames if (k == 0 and w == 0) else synth_frames([rank * 1000 + 100 * (k * W + w) + i for i in range(T)]).to(dev)
                 for w in range(W)]
        return clips[0] if W == 1 else torch.cat(clips, 0)
    frames_w = lane_frames(0)
    metas_w = metas * W
    if args.lanes <= 0:   # auto: every round of replays fills every lane (profiles/r05_lanes.txt: a partial last round costs 2-4 %)
        replays = args.steps // W
        args.lanes = next((l for l in (4, 5, 6, 3) if replays % l == 0), 4)

    lanes = [torch.cuda.Stream(device=dev) for _ in range(max(1, args.inflight))] if args.inflight > 1 else [None]
    turn = [0]
    last_call = [None]   # every clip's result of the last call a timed region read (--dump-outputs)

    def read_all(pend):
        """result() of one pending window or of the W windows of a batched call -> [every clip's result]"""
        if isinstance(pend, list):
            return [p_.result() for p_ in pend]
        return [pend.result()]

    def read(pend):
        """result() of one pending window or of the W windows of a batched call -> the first clip's result"""
        return read_all(pend)[0]

    def step(prev=None, w=1):
        """Enqueues one call -- one window, or w > 1 independent clips as one batch (detectors.forward_feat_clips) -- and collects
        the PREVIOUS call's results afterwards (its single host sync), so the host is never waiting on the work it has just
        launched.  Every window's results are read inside the timed region.
        With --inflight N > 1 consecutive windows go to N HIP streams in turn: they are independent clips, and the
        latency-bound phases of one (proposals, read-out) run under the dense phases of another."""
        lane = lanes[turn[0] % len(lanes)]
        turn[0] += 1
        with torch.no_grad(), (torch.cuda.stream(lane) if lane is not None else contextlib.nullcontext()):
            if w > 1:
                c4 = model(img=frames_w, img_meta=metas_w, backbone_feat=True)[0]   # backbone on all W * T frames
                pend = model.forward_feat_clips(c4, metas_w, clips=w, rescale=True, defer=True)
            else:
                c4 = model(img=frames, img_meta=metas, backbone_feat=True)[0]       # backbone on all T frames
                pend = model(x=c4, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True, defer=True)
        if prev is not None:
            read(prev)
        return pend

    def sync():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def over_ranks(seconds):
        """-> (max over ranks, every rank's own time)"""
        if world == 1:
            return seconds, [seconds]
        t = torch.tensor([seconds], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        allt = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(allt, torch.tensor([seconds], dtype=torch.float64, device=dev))
        return float(t.item()), [float(x.item()) for x in allt]

    def timed(steps, warmup, tags=None, w=1):
        """`steps` windows as steps / w calls of w clips each"""
        pend = None
        for _ in range(max(1, warmup // w) if warmup else 0):
            pend = step(pend, w)
        if pend is not None:
            read(pend)
        sync()
        if tags:
            native.profile_begin(tags=tags)
        t0 = time.perf_counter()
        pend = None
        for _ in range(steps // w):
            pend = step(pend, w)
        last_call[0] = read_all(pend)
        res = last_call[0][0]
        sync()
        el = time.perf_counter() - t0
        spans = native.profile_end() if tags else None
        return el, res, spans

    def graph_regions(n_lanes, steps, warmup, repeats, w=1):
        """K windows replayed from hipGraphs (one graph per w clips, captured in the model's current compute mode, every lane and clip
        with frames of its own) on n_lanes HIP streams in turn, the region timed `repeats` times -> ([seconds per region], the result
        of lane 0's first clip = `frames`)."""
        from hvrnet_amd.graphs import GraphedClip
        lane_streams = [torch.cuda.Stream(device=dev) for _ in range(n_lanes)]
        gcs = []
        for k, st in enumerate(lane_streams):
            with torch.cuda.stream(st):
                gcs.append(GraphedClip(model, lane_frames(k) if w == W else frames, metas * w, rescale=True, n_out=1, throughput=n_lanes > 1, windows=w))
        pend_l = [None] * n_lanes
        lane_out = [None] * n_lanes
        first = [None]

        def collect(k):
            if pend_l[k] is not None:
                lane_out[k] = read_all(pend_l[k])
                if k == 0:
                    first[0] = lane_out[k][0]
                pend_l[k] = None

        def replay(i):
            k = i % n_lanes
            collect(k)   # a lane's previous windows are read before its buffers are reused
            with torch.cuda.stream(lane_streams[k]):
                pend_l[k] = gcs[k].run()

        def drain():
            for k in range(n_lanes):
                collect(k)

        for i in range(max(warmup // w, n_lanes)):
            replay(i)
        drain()
        times = []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            for i in range(steps // w):
                replay(i)
            drain()
            sync()
            times.append(time.perf_counter() - t0)
        if repeats and steps // w:
            last_call[0] = lane_out[(steps // w - 1) % n_lanes]
        del gcs
        return times, first[0]

    def roofline_of(mode, rel_spans, units=1):
        """The relation core's calls (hvr_relation_fwd[_grouped] with Mq = Mk = T x proposals, D = 1024: 4 Mq Mk D flops per window;
        f16x2: three half MFMAs per product, so its peak is the half peak / 3), HIP events around every call on the launch stream in an
        eager one-call-in-flight region.  units = windows per call (`units_per_launch`: a grouped call covers the W clips of a batched
        window; `avg_ms` is per CALL, `ms_per_unit` per window); `traffic`: HBM-side bytes per window from the committed PMC passes of
        THIS library build, else null."""
        full = (rel_spans or {}).get('relation_full', dict(calls=0, ms=0.0, work=0.0))
        if not full['calls']:
            return None
        peak = MFMA_PEAK_TF[mode]
        ach = full['work'] / (full['ms'] * 1e-3) / 1e12
        traffic = relation_traffic(units, mode)[0] if T * n_prop == 4500 and mode in ('bf16', 'f16x2') else None
        return dict(kernel='relation core', bound='mfma', achieved=round(ach, 2), peak=round(peak, 1), unit='TFLOP/s', frac=round(ach / peak, 4),
                    traffic=traffic, launches=full['calls'], avg_ms=round(full['ms'] / full['calls'], 4), units_per_launch=units,
                    ms_per_unit=round(full['ms'] / full['calls'] / units, 4), flops_per_launch=full['work'] / full['calls'])

    def class_times(mode, w=1):
        """One extra instrumented call of w clips (outside every timed region): per kernel class [ms PER WINDOW, fraction of the mode's
        MFMA peak or of the HBM peak]."""
        # the backbone / RPN / res5 part as ONE chain (no RPN side stream): with a branch on another stream the HIP-event interval around
        # a call is the time its launch shared the chip with that branch's, not the kernel's own (round 4's "328 us" RPN heads: 23 us alone)
        undo = []
        for obj, attr in ((model, 'rpn_side_stream'),):
            if getattr(obj, attr, False):
                setattr(obj, attr, False)
                undo.append((obj, attr))
        try:
            read(step(None, w))   # (first call of this form: scratch buffers of the main stream may grow)
            torch.cuda.synchronize()
            native.profile_begin(tags=('*',))
            read(step(None, w))
            spans = native.profile_end()
        finally:
            for obj, attr in undo:
                delattr(obj, attr)   # back to the class attribute
        out_c, peak_m = {}, MFMA_PEAK_TF[mode]
        for tag, d in spans.items():
            if d['ms'] <= 0:
                continue
            mfma = tag in ('gemm', 'conv', 'stem', 'relation_full', 'relation_key')
            rate = d['work'] / (d['ms'] * 1e-3) / (1e12 if mfma else 1e9)
            out_c[tag] = dict(calls=d['calls'], ms=round(d['ms'] / w, 4), frac=round(rate / (peak_m if mfma else HBM_PEAK_GBS), 4), of='mfma' if mfma else 'hbm')
        return out_c

    median = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    eager_mode = 'eager launches, %d window(s) in flight'
    graph_mode = 'hipGraph replay (one graph per %d independent clip(s), distinct frames per lane and clip), %d windows in flight on %d HIP streams'

    def headline_figures(region_times):
        """per region the slowest rank counts; the reported region is the median one -> (seconds, every rank's own, value_spread)"""
        per_region = [over_ranks(t_) for t_ in region_times]
        order = sorted(range(len(per_region)), key=lambda i: per_region[i][0])
        elapsed, per_rank = per_region[order[len(order) // 2]]
        value_spread = dict(regions=len(per_region), frames_per_s=[round(world * args.steps / t_[0], 2) for t_ in per_region],
                            rel_spread=round((max(t_[0] for t_ in per_region) - min(t_[0] for t_ in per_region)) / elapsed, 4))
        return elapsed, per_rank, value_spread

    def contract_keys(elapsed, n_lanes, headline_mode, res):
        """the head of the JSON line: the contract keys and the headline's configuration"""
        branch = res[-1] if args.head == 'hvr' else res
        n_det = int(sum(len(r) for r in branch))
        return dict(metric='VID frames/sec, R101 Faster-RCNN+%s, 1000x600, %d props, T=%d' % (args.head.upper(), n_prop, T),
                    value=round(world * args.steps / elapsed, 3), unit='frames/s', n_gpus=world, steps=args.steps, warmup=args.warmup,
                    ms_per_step=round(elapsed / args.steps * 1e3, 3), higher_is_better=True, scaling='weak', vs_baseline=None,
                    dtype=args.dtype, data='synthetic',
                    config=dict(workload='configs[2]: faster_rcnn_r101_hrnmp_c5 inference, clip mode' if args.head == 'hvr'
                                else 'configs[1]: faster_rcnn_r101_selsa_c5 inference, clip mode',
                                frames_per_window=T, proposals_per_frame=n_prop, input='3x600x1000 padded to 608x1008',
                                parallelism='dp%d independent clips, no collectives' % world, windows_in_flight=n_lanes * (W if headline_mode.startswith('hipGraph') else 1), clips_per_graph=W, launch=headline_mode,
                                key_frame_detections=n_det))

    def closing_keys(out, per_rank):
        out['gpus_requested'] = args.gpus
        out['per_rank'] = [dict(rank=i, frames_per_s=round(args.steps / t_, 3)) for i, t_ in enumerate(per_rank)]
        out['rccl_world_size'] = dist.get_world_size() if world > 1 else 1
        prop = torch.cuda.get_device_properties(dev)
        out['device'] = dict(name=prop.name, cus=prop.multi_processor_count, hbm_gb=round(prop.total_memory / 2 ** 30, 1))
        out['lib_sha16'] = lib_sha16()

    if not args.full:
        # ---- a plain run: the headline region alone -- set-up, warm-up, the K timed steps (`repeats` times, default once) and the
        # contract keys; everything else this file measures or checks runs with --full ----
        if args.lanes > 1 and not args.no_graphs and args.inflight == 1:
            n_lanes = args.lanes
            region_times, res = graph_regions(n_lanes, args.steps, args.warmup, max(1, args.repeats), W)
            headline_mode = graph_mode % (W, n_lanes * W, n_lanes)
        else:
            n_lanes = max(1, args.inflight)
            region_times = []
            for r in range(max(1, args.repeats)):
                el, res, _ = timed(args.steps, args.warmup if r == 0 else 1)
                region_times.append(el)
            headline_mode = eager_mode % n_lanes
        elapsed, per_rank, value_spread = headline_figures(region_times)
        if rank == 0:
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, last_call[0], args.head)
            out = contract_keys(elapsed, n_lanes, headline_mode, res)
            out['value_spread'] = value_spread
            closing_keys(out, per_rank)
            print(json.dumps(out, separators=(',', ':')))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- region (1): the eager single-lane loop, relation launches tagged; timed `repeats` times (at least 3) ----
    sl_times, rel = [], {}
    for r in range(max(1, min(args.repeats, 3))):
        el, res, spans = timed(args.steps, args.warmup if r == 0 else 1, tags=('relation_full', 'relation_key'))
        sl_times.append(el)
        for tag, d in spans.items():
            e = rel.setdefault(tag, dict(calls=0, ms=0.0, work=0.0))
            e['calls'] += d['calls']; e['ms'] += d['ms']; e['work'] += d['work']
    mine = median(sl_times)
    single_lane = dict(frames_per_s=round(args.steps / mine, 3), ms_per_step=round(mine / args.steps * 1e3, 3), steps=args.steps,
                       regions=[round(args.steps / t_, 2) for t_ in sl_times],
                       rel_spread=round((max(sl_times) - min(sl_times)) / mine, 4))
    rel_single = rel
    res_single = res   # the eager one-window-per-call result of `frames` (what a one-clip graph has to reproduce bit for bit)
    head_last = last_call[0]
    # ---- region (1b): the same loop with W clips per call (what a graph of the headline region holds): the relation core's grouped
    # calls tagged -- `roofline` is taken HERE when W > 1 (units_per_launch = W), the one-window region above stays as `roofline_one_window` ----
    batched_lane, batched_vs_single = None, {}
    if W > 1:
        b_times, rel = [], {}
        for r in range(2):
            el, res, spans = timed(args.steps, W, tags=('relation_full', 'relation_key'), w=W)
            b_times.append(el)
            for tag, d in spans.items():
                e = rel.setdefault(tag, dict(calls=0, ms=0.0, work=0.0))
                e['calls'] += d['calls']; e['ms'] += d['ms']; e['work'] += d['work']
        bm = min(b_times)
        batched_lane = dict(frames_per_s=round(args.steps / bm, 3), ms_per_step=round(bm / args.steps * 1e3, 3), steps=args.steps, clips_per_call=W)
        batched_vs_single = {args.dtype: clip_distance(args.head, res, res_single)}   # clip 0 of the W-clip call against the one-window call
    headline_mode = eager_mode % max(1, args.inflight)
    n_lanes = max(1, args.inflight)
    region_times = sl_times
    if args.lanes > 1 and not args.no_graphs and args.inflight == 1:
        # ---- headline region: K windows replayed from hipGraphs on `lanes` HIP streams in turn, timed `repeats` times ----
        n_lanes = args.lanes
        region_times, res = graph_regions(n_lanes, args.steps, args.warmup, max(1, args.repeats), W)
        headline_mode = graph_mode % (W, n_lanes * W, n_lanes)
        head_last = last_call[0]
    elapsed, per_rank, value_spread = headline_figures(region_times)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, head_last, args.head)

    # ---- the precision ladder: the same window in the other compute modes (rank 0, N = 1) ----
    ladder = {}
    if not args.no_f32_leg and world == 1:
        for mode in [m for m in args.ladder.split(',') if m and m != args.dtype]:
            hvrnet_amd.set_compute_dtype(model, MODES[mode])
            n_m = max(2, min(args.steps, 5 if mode == 'f32' else 10))
            n_m = (n_m + W - 1) // W * W
            el_m, res_m, spans_m = timed(n_m, W, tags=('relation_full', 'relation_key'), w=W)
            row = dict(dtype=mode, single_lane=dict(frames_per_s=round(n_m / el_m, 3), ms_per_step=round(el_m / n_m * 1e3, 3), steps=n_m, clips_per_call=W),
                       roofline=roofline_of(mode, spans_m, W), kernel_classes=class_times(mode, W))
            if W > 1:
                batched_vs_single[mode] = clip_distance(args.head, res_m, read(step(None, 1)))
            if args.lanes > 1 and not args.no_graphs and args.inflight == 1:
                n_g = args.lanes * W * (2 if mode == 'f32' else 3)   # whole rounds of the lanes (a partial last round is idle lanes, not the mode), >= 0.3 s per region
                tg, res_g = graph_regions(args.lanes, n_g, 2, 3, W)
                tg_m = median(tg)   # (three regions, the median: one region of a few hundred ms moves by 2-3 % with the clocks)
                row['graph_replay'] = dict(frames_per_s=round(n_g / tg_m, 3), ms_per_step=round(tg_m / n_g * 1e3, 3), steps=n_g, lanes=args.lanes)
                row['_res'] = res_g
            else:
                row['_res'] = res_m
            ladder[mode] = row
        hvrnet_amd.set_compute_dtype(model, dt)
    ref_loop_fps = cached_loop_fps = overlap2_fps = None
    n_loop = max(3, min(args.steps, 10))
    if not args.no_side_loops:
        # the reference's own steady-state loop (tools/test.py:214-250): ONE new frame through the backbone per output
        # frame, the other T-1 C4 maps come from the deque; reported next to the clip-mode headline, never as `value`
        with torch.no_grad():
            c4_all = model(img=frames, img_meta=metas, backbone_feat=True)[0]
            window = [c4_all[i:i + 1] for i in range(T)]
        sync()
        t1 = time.perf_counter()
        for i in range(n_loop):
            with torch.no_grad():
                new = model(img=frames[i % T:i % T + 1], img_meta=[metas[0]], backbone_feat=True)[0]
                window = window[1:] + [new]
                model(x=window, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
        sync()
        ref_loop_fps = n_loop / (time.perf_counter() - t1)

        # the same loop with the per-frame cache: res5 / RPN / RoIAlign / fc_new_1 run once per incoming frame
        # (model.frame_tensors), a window runs the relation stages and the read-out on the T cached entries; the results
        # are bit-identical to the two loops above (tests/test_parity_gpu.py::test_cached_frame_loop_matches_clip_mode)
        with torch.no_grad():
            entries = [model.frame_tensors(c, m) for c, m in zip(window, metas)]
        sync()
        t2 = time.perf_counter()
        pend = None
        for i in range(n_loop):
            with torch.no_grad():
                new = model(img=frames[i % T:i % T + 1], img_meta=[metas[0]], backbone_feat=True)[0]
                window = window[1:] + [new]
                entries = entries[1:] + [model.frame_tensors(new, metas[0])]
                nxt = model.forward_feat_frames(entries, c4s=window, rescale=True, defer=True)
            if pend is not None:
                pend.result()
            pend = nxt
        pend.result()
        sync()
        cached_loop_fps = n_loop / (time.perf_counter() - t2)

        # clip mode again with TWO independent windows in flight on two HIP streams (frame groups off): the latency-bound
        # phases of one window (proposals, read-out) run under the dense phases of the other.  Reported beside the headline:
        # the headline run stays single-lane so that the HIP-event times around the relation core are that kernel's own
        if args.inflight == 1 and world == 1:
            lanes[:] = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
            n2 = max(4, min(args.steps, 12))
            el2, _, _ = timed(n2, 2)
            overlap2_fps = n2 / el2
            overlap2 = dict(frames_per_s_per_gpu=round(overlap2_fps, 2), steps=n2, elapsed_ms=round(el2 * 1e3, 3))
            lanes[:] = [None]

    # ---- frame ingest inside the loop: every frame of every window starts as a uint8 BGR frame on the
    # device (600 x 1000 x 3: the decoded frame a host would hand over, 1.8 MB instead of the 7.3 MB f32 tensor) and goes through
    # hvr_ingest_frame (resize arithmetic, mean / std, zero pad to /16, HWC -> CHW) before the window -- the same eager W-clips-per-call loop
    # as `single_lane_batched`, which starts from resident f32 tensors.  A side figure, never `value`.
    ingest_loop = None
    if not args.no_side_loops and world == 1:
        from hvrnet_amd.pipelines import FrameIngest
        ing = FrameIngest(device=dev)
        gen = torch.Generator().manual_seed(7)
        src = [torch.randint(0, 256, (600, 1000, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(T * W)]

        def step_ingest(prev=None):
            with torch.no_grad():
                imgs = torch.cat([ing(f)['img'] for f in src], 0)
                c4_i = model(img=imgs, img_meta=metas_w, backbone_feat=True)[0]
                pend_i = model.forward_feat_clips(c4_i, metas_w, clips=W, rescale=True, defer=True)
            if prev is not None:
                read(prev)
            return pend_i
        assert tuple(ing(src[0])['img'].shape) == tuple(frames[0:1].shape)
        pend = step_ingest()
        read(step_ingest(pend))
        sync()
        n_i = max(W, (min(args.steps, 12) // W) * W)
        t_i = time.perf_counter()
        pend = None
        for _ in range(n_i // W):
            pend = step_ingest(pend)
        read(pend)
        sync()
        el_i = time.perf_counter() - t_i
        ingest_loop = dict(frames_per_s=round(n_i / el_i, 2), ms_per_step=round(el_i / n_i * 1e3, 3), steps=n_i, elapsed_ms=round(el_i * 1e3, 3), clips_per_call=W,
                           source='uint8 600x1000x3 frames resident on the device, hvr_ingest_frame per frame inside the loop')

    # ---- the same work replayed from hipGraphs (hvrnet_amd/graphs.py): the window / the per-frame and per-window chains are
    # captured once, with their side streams, and replayed with one host call each.  Reported beside the eager headline (whose
    # per-kernel HIP-event spans cannot be taken inside a replay); bit-identical detections (tests/test_graphs_gpu.py).
    graphed_clip = graphed_stream = None
    if not args.no_graphs and args.inflight == 1:
        from hvrnet_amd.graphs import GraphedClip, GraphedStream
        gc = GraphedClip(model, frames, metas, rescale=True)
        pend = gc.run()
        pend.result()
        sync()
        ng = max(4, args.steps)
        tg = time.perf_counter()
        pend = None
        for _ in range(ng):
            nxt = gc.run()
            if pend is not None:
                pend.result()
            pend = nxt
        res_graph = pend.result()
        sync()
        el = time.perf_counter() - tg
        graphed_clip = dict(frames_per_s_per_gpu=round(ng / el, 3), ms_per_step=round(el / ng * 1e3, 3), steps=ng,
                            same_detections=same_detections(res_graph, res_single))   # one-clip graph vs the eager one-window call: like with like
        del gc
        # stream mode: one new frame per output frame, per-frame cache, graph F (frame arrives) + graph W (window emitted)
        gs = GraphedStream(model, frames[0:1], metas[0], rescale=True)
        for i in range(T):
            gs.push(frames[i:i + 1])
        gs.emit().result()
        sync()
        nsg = max(10, args.steps)
        tg = time.perf_counter()
        pend = None
        for i in range(nsg):
            gs.push(frames[i % T:i % T + 1])
            nxt = gs.emit()
            if pend is not None:
                pend.result()
            pend = nxt
        pend.result()
        sync()
        el = time.perf_counter() - tg
        gf = 650.0 if args.head == 'hvr' else 504.0
        graphed_stream = dict(frames_per_s_per_gpu=round(nsg / el, 2), ms_per_frame=round(el / nsg * 1e3, 3), steps=nsg,
                              tflops=round(nsg / el * gf / 1e3, 1), frac_mfma_peak=round(nsg / el * gf / 1e3 / MFMA_PEAK_TF[args.dtype], 4))
        # the same loop pipelined: frame i + 1's per-frame part (graph FC on a second stream) runs beside window i's relation
        # stages and read-out; one frame arrives per output frame, nothing is batched
        gs.push_async(frames[0:1])
        for i in range(T):
            gs.commit()
            gs.push_async(frames[(i + 1) % T:(i + 1) % T + 1])
            gs.emit().result()
        sync()
        tg = time.perf_counter()
        pend = None
        for i in range(nsg):
            gs.commit()
            gs.push_async(frames[(i + 2) % T:(i + 2) % T + 1])
            nxt = gs.emit()
            if pend is not None:
                pend.result()
            pend = nxt
        pend.result()
        gs.commit()
        sync()
        el = time.perf_counter() - tg
        graphed_stream['pipelined'] = dict(frames_per_s_per_gpu=round(nsg / el, 2), ms_per_frame=round(el / nsg * 1e3, 3), steps=nsg,
                                           tflops=round(nsg / el * gf / 1e3, 1), frac_mfma_peak=round(nsg / el * gf / 1e3 / MFMA_PEAK_TF[args.dtype], 4))
        del gs
        # the same loop with look-ahead batches (offline video: T frames through the per-frame part at once, then one output frame
        # at a time): what a single 600x1000 frame cannot give the chip -- 2 394 stride-16 rows are 17-19 row tiles for 256 CUs
        gl = GraphedStream(model, frames[0:1], metas[0], rescale=True, lookahead=T)
        gl.push_batch(frames)
        for i in range(T):
            gl.advance(i)
        gl.emit().result()
        sync()
        nb = max(2, args.steps // 5)
        tg = time.perf_counter()
        pend = None
        for b in range(nb):
            gl.push_batch(frames)
            for i in range(T):
                gl.advance(i)
                nxt = gl.emit()
                if pend is not None:
                    pend.result()
                pend = nxt
        pend.result()
        sync()
        el = time.perf_counter() - tg
        graphed_stream['lookahead'] = dict(frames_per_s_per_gpu=round(nb * T / el, 2), ms_per_frame=round(el / (nb * T) * 1e3, 3), batch=T,
                                           steps=nb * T, tflops=round(nb * T / el * gf / 1e3, 1),
                                           frac_mfma_peak=round(nb * T / el * gf / 1e3 / MFMA_PEAK_TF[args.dtype], 4))
        del gl

    # per-class breakdown from one extra, fully instrumented window (outside the timed region)
    kc = class_times(args.dtype, W)
    if args.breakdown and rank == 0:
        native.profile_begin(tags=('*',), detail=True)
        read(step(None, W))
        for tag, d in sorted(native.profile_end().items(), key=lambda kv: -kv[1]['ms']):
            rate = d['work'] / (d['ms'] * 1e-3) / 1e12 if d['ms'] > 0 else 0.0
            sys.stderr.write('%-44s calls %3d  %8.3f ms  %8.1f T(FLOP|B)/s\n' % (tag, d['calls'], d['ms'], rate))

    ar = allreduce_leg(dist, world, args.head, dev) if world > 1 else None

    if rank == 0:
        # The line is ordered for a reader of its first kilobytes: the contract keys, then the figure that carries north_star's tolerance
        # (`within_tolerance`), the steering figure (`single_lane`), `roofline`, `cpu_baseline`, the ladder; side loops last.  What each
        # key means is in README.md ("Reading the bench line"); the line itself carries numbers.
        peak = MFMA_PEAK_TF[args.dtype]
        roofline = roofline_of(args.dtype, rel, W)
        roofline_one = roofline_of(args.dtype, rel_single, 1) if W > 1 else None
        out = contract_keys(elapsed, n_lanes, headline_mode, res)
        want = None
        cpu = None
        wants, wants64, noise_floor, want_props = [], [], None, []
        # clips the tolerance is checked on: the benchmark's + seven more (other synthetic frames, same weights) -- VERDICT r05 item 1b
        tol_clip_ids = [frame_ids] + [[rank * 1000 + 5000 * c + i for i in range(T)] for c in range(1, max(1, args.tol_clips))]
        if world == 1 and not args.no_cpu_baseline:
            if args.quick:
                cpu, want = cpu_baseline_quick(args.head, T, n_prop, sd)
            else:
                cpu, wants, wants64, noise_floor, want_props = cpu_baseline_full(args.head, T, n_prop, sd, tol_clip_ids)
                want = wants[0]
        # ---- the precision ladder: every compute mode's throughput next to how far its detections are from the CPU reference path ----
        sl_row = batched_lane or single_lane
        head_row = dict(dtype=args.dtype, headline=True, single_lane=dict(frames_per_s=sl_row['frames_per_s'], ms_per_step=sl_row['ms_per_step'],
                                                                         steps=args.steps, clips_per_call=W), roofline=roofline, kernel_classes=kc)
        if headline_mode.startswith('hipGraph'):
            head_row['graph_replay'] = dict(frames_per_s=out['value'], ms_per_step=out['ms_per_step'], steps=args.steps, lanes=n_lanes)
        head_row['_res'] = res
        rows = [head_row] + list(ladder.values())
        for row in rows:
            if want is not None:
                row['parity'] = parity_object(args.head, row['dtype'], row.pop('_res'), want)
                row['within_tolerance'] = within_tolerance(row['parity'])
            else:
                row.pop('_res', None)
        # a mode whose classes and scores agree with the reference on the benchmark's clip is checked on EVERY clip (one eager window
        # each) against the oracle's f32 evaluation -- `within_tolerance` is the claim over ALL clips, none left out by a rule of this
        # file (VERDICT r05 item 1c / ADVICE r05): a clip whose RPN proposal lists equal the oracle's has to be inside the bar as it is;
        # a clip whose lists differ (an NMS pair at the IoU threshold resolved differently by two f32 evaluations) FAILS the claim unless
        # (i) the same window with the oracle's proposal lists injected is inside the bar and (ii) every differing frame's decision at
        # issue is an NMS pair within parity.NMS_TIE_BAND of the threshold (the pair and its float64 IoU are in the record).
        # Beside it: the distances to the oracle's f64 evaluation, round 4's fixed bar, and north_star's figure read literally (1e-3 px).
        if len(wants) > 1:
            from hvrnet_amd import parity as _par
            for row in rows:
                pr0 = row['parity']
                if pr0['class_flips'] != 0 or not pr0['max_score_err'] < TOL_SCORE:
                    continue
                hvrnet_amd.set_compute_dtype(model, MODES[row['dtype']])
                p32, p64, same_props, injected, ties, passes = [], [], [], [], [], []
                for ci, (ids, w32, wp) in enumerate(zip(tol_clip_ids, wants, want_props)):
                    w64 = wants64[ci] if ci < len(wants64) else None
                    fr_c = frames if ids is tol_clip_ids[0] else torch.cat([S.synth_frame(i) for i in ids], 0).to(dev)
                    with torch.no_grad():
                        c4_c = model(img=fr_c, img_meta=metas, backbone_feat=True)[0]
                        got_c = model(x=c4_c, img=None, img_meta=metas, forward_feat=True, return_loss=False, rescale=True)
                        dev_props = [p_.cpu().numpy() for p_ in model.window_tensors(c4_c, metas)['proposals']]
                    p32.append(parity_object(args.head, row['dtype'], got_c, w32))
                    p64.append(parity_object(args.head, row['dtype'], got_c, w64) if w64 is not None else None)
                    sp = all(_par.proposal_lists_equal(dev_props, wp))
                    same_props.append(bool(sp))
                    if sp:
                        injected.append(None)
                        passes.append(within_tolerance(p32[-1]))
                    else:
                        with torch.no_grad():
                            got_i = model(x=c4_c, img=None, img_meta=metas, proposals=[torch.from_numpy(p_).to(dev) for p_ in wp],
                                          forward_feat=True, return_loss=False, rescale=True)
                        pi = parity_object(args.head, row['dtype'], got_i, w32)
                        tl = _par.nms_threshold_ties(dev_props, wp, thr=0.7)
                        injected.append(dict(class_flips=pi['class_flips'], max_score_err=pi['max_score_err'], max_box_err=pi['max_box_err'],
                                             within_tolerance=within_tolerance(pi), literal_1e3=_par.literal_1e3(pi)))
                        ties.append(dict(clip=ci, frames=[dict(frame=t_['frame'], kept_by='device' if t_['side'] == 'got' else 'oracle', iou_f64=t_['iou'],
                                                             box=t_['box'], suppressor=t_['suppressor'], is_tie=t_['is_tie']) for t_ in tl]))
                        passes.append(bool(within_tolerance(pi) and len(tl) > 0 and all(t_['is_tie'] for t_ in tl)))
                row['parity_clips'] = dict(clips=len(p32), passes=passes, class_flips=[p_['class_flips'] for p_ in p32], tie_swaps=[p_['tie_swaps'] for p_ in p32],
                                           max_score_err=[p_['max_score_err'] for p_ in p32], max_box_err_vs_f32=[p_['max_box_err'] for p_ in p32],
                                           max_box_excess_vs_f32=[p_['max_box_excess'] for p_ in p32],
                                           max_box_err_vs_f64=[p_['max_box_err'] for p_ in p64 if p_ is not None],
                                           fixed_bar_r04=[_par.fixed_bar_r04(p_) for p_ in p32],
                                           literal_1e3_vs_f32=[_par.literal_1e3(p_) for p_ in p32], literal_1e3_vs_f64=[_par.literal_1e3(p_) for p_ in p64 if p_ is not None],
                                           proposal_lists_equal_the_oracles=same_props, with_the_oracles_proposals_injected=injected, nms_threshold_ties=ties)
                row['within_tolerance'] = bool(all(passes))
            hvrnet_amd.set_compute_dtype(model, dt)
        ok = [r for r in rows if r.get('within_tolerance')]
        if ok:
            best = max(ok, key=lambda r: (r.get('graph_replay') or r['single_lane'])['frames_per_s'])
            fig = best.get('graph_replay') or best['single_lane']
            pc = best.get('parity_clips')
            if pc:
                cnt = pc['proposal_lists_equal_the_oracles']
                mx = (lambda key: max(v for v, sp in zip(pc[key], cnt[:len(pc[key])]) if sp))   # over the clips checked as they are
                inj = [i_ for i_ in pc['with_the_oracles_proposals_injected'] if i_ is not None]
                worst = dict(class_flips=mx('class_flips'), max_score_err=mx('max_score_err'), max_box_err=mx('max_box_err_vs_f32'),
                             max_box_excess=mx('max_box_excess_vs_f32'), max_box_err_vs_f64=(max([v for v, sp in zip(pc['max_box_err_vs_f64'], cnt) if sp] or [None]) if pc['max_box_err_vs_f64'] else None),   # (over the f64 clips checked as they are)
                             tie_swaps=mx('tie_swaps'), max_box_err_with_injected_proposals=max([i_['max_box_err'] for i_ in inj]) if inj else None,
                             fixed_bar_r04_on_every_clip_checked_as_it_is=all(f_ for f_, sp in zip(pc['fixed_bar_r04'], cnt) if sp),
                             literal_1e3_px=dict(vs_f32=[sum(pc['literal_1e3_vs_f32']), pc['clips']], vs_f64=[sum(pc['literal_1e3_vs_f64']), len(pc['literal_1e3_vs_f64'])]))
            else:
                worst = dict(class_flips=best['parity']['class_flips'], max_score_err=best['parity']['max_score_err'], max_box_err=best['parity']['max_box_err'])
            out['within_tolerance'] = dict(dtype=best['dtype'], frames_per_s=fig['frames_per_s'], ms_per_step=fig['ms_per_step'],
                                           lanes=fig.get('lanes', 1), clips_per_graph=W, single_lane_frames_per_s=best['single_lane']['frames_per_s'],
                                           roofline=best['roofline'], parity=worst, clips_checked=pc['clips'] if pc else 1,
                                           clips_passed=sum(pc['passes']) if pc else 1,
                                           clips_with_the_oracles_proposal_lists=sum(pc['proposal_lists_equal_the_oracles']) if pc else None,
                                           clips_proven_by_injection=sum(1 for i_ in pc['with_the_oracles_proposals_injected'] if i_ is not None) if pc else None,
                                           per_clip=dict(max_box_err_vs_f64=pc['max_box_err_vs_f64'], max_box_err_vs_f32=pc['max_box_err_vs_f32'],
                                                         literal_1e3_vs_f32=pc['literal_1e3_vs_f32'], literal_1e3_vs_f64=pc['literal_1e3_vs_f64'],
                                                         proposal_lists_equal_the_oracles=pc['proposal_lists_equal_the_oracles'],
                                                         with_the_oracles_proposals_injected=pc['with_the_oracles_proposals_injected'],
                                                         nms_threshold_ties=pc['nms_threshold_ties']) if pc else None,
                                           oracle_noise_floor=noise_floor,
                                           tolerance=dict(class_flips=0, score=TOL_SCORE, box_px=TOL_BOX_PX, box_rtol=BOX_RTOL, nms_tie_band=_par.NMS_TIE_BAND if pc else None,
                                                          defined='hvrnet_amd/parity.py (frozen since round 5)'))
        elif want is not None:
            out['within_tolerance'] = None
        if want is not None:
            # every mode that agreed with the reference on the benchmark clip and FAILED the claim over all clips, with the reason -- also when a
            # slower mode carries the claim (a faster mode's failure is not to disappear behind it)
            fails = [dict(dtype=r['dtype'], **{k_: r['parity_clips'][k_] for k_ in ('passes', 'max_box_err_vs_f32', 'proposal_lists_equal_the_oracles',
                                                                              'with_the_oracles_proposals_injected', 'nms_threshold_ties')})
                     for r in rows if 'parity_clips' in r and not r.get('within_tolerance')]
            if fails:
                out['within_tolerance_failed'] = fails
        out['single_lane'] = single_lane
        if batched_lane is not None:
            out['single_lane_batched'] = batched_lane
        out['roofline'] = roofline
        if roofline_one is not None:
            out['roofline_one_window'] = dict(frac=roofline_one['frac'], avg_ms=roofline_one['avg_ms'], achieved=roofline_one['achieved'], launches=roofline_one['launches'])
        if cpu is not None:
            out['cpu_baseline'] = cpu
        out['value_spread'] = value_spread
        if batched_vs_single:
            out['batched_vs_single'] = batched_vs_single
        if want is not None:
            pr = head_row['parity']
            out['parity'] = dict(dtype=pr['dtype'], class_flips=pr['class_flips'], max_score_err=pr['max_score_err'], max_box_err=pr['max_box_err'],
                                 detections=pr['detections'], same_class_frac=pr['matched']['same_class_frac'], within_tolerance=head_row['within_tolerance'])
        if ladder or want is not None:
            # one compact row per compute mode: eager = [frames/s, ms] of the single-lane loop, replay = [frames/s, ms, lanes] of the
            # headline's launch mode, kernel_classes = class -> [ms, fraction of that mode's MFMA peak or of the HBM peak]
            def compact(r):
                c = dict(dtype=r['dtype'], eager=[r['single_lane']['frames_per_s'], r['single_lane']['ms_per_step']])
                if r.get('headline'):
                    c['headline'] = True
                if 'graph_replay' in r:
                    c['replay'] = [r['graph_replay']['frames_per_s'], r['graph_replay']['ms_per_step'], r['graph_replay']['lanes']]
                rf = r.get('roofline')
                c['roofline'] = dict(bound='mfma', achieved=rf['achieved'], peak=rf['peak'], unit=rf['unit'], frac=rf['frac'], avg_ms=rf['avg_ms']) if rf else None
                if 'parity' in r:
                    pr = r['parity']
                    c['parity'] = dict(class_flips=pr['class_flips'], max_score_err=pr['max_score_err'], max_box_err=pr['max_box_err'],
                                       same_class_frac=pr['matched']['same_class_frac'])
                    c['within_tolerance'] = r['within_tolerance']
                    if 'parity_clips' in r:   # (the per-clip arrays of the mode that carries the claim are in `within_tolerance`)
                        pc_ = r['parity_clips']
                        c['clips'] = [sum(pc_['passes']), pc_['clips']]
                c['kernel_classes'] = {t: [round(e['ms'], 3), round(e['frac'], 3)] for t, e in r['kernel_classes'].items()}
                return c
            out['precision_ladder'] = [compact(r) for r in rows]
        out['kernel_classes'] = kc
        closing_keys(out, per_rank)
        if ref_loop_fps is not None:
            out['ref_loop'] = dict(frames_per_s_per_gpu=round(ref_loop_fps, 2), steps=n_loop)
            # ~650 GF (HVR) / 504 GF (SELSA) per output frame with the per-frame cache (SURVEY.md 8d "stream mode")
            gf = 650.0 if args.head == 'hvr' else 504.0
            out['cached_loop'] = dict(frames_per_s_per_gpu=round(cached_loop_fps, 2), steps=n_loop,
                                      tflops=round(cached_loop_fps * gf / 1e3, 1), frac_mfma_peak=round(cached_loop_fps * gf / 1e3 / peak, 4))
        if overlap2_fps is not None:
            out['two_in_flight'] = overlap2
        if ingest_loop is not None:
            out['ingest_in_loop'] = ingest_loop
        if graphed_clip is not None:
            out['graphed_clip'] = graphed_clip
            out['graphed_stream'] = graphed_stream
        if ar is not None:
            # what the first real multi-GPU training run should see: the HVR step is ~21.9 ms on one GPU (profiles/r02_train_bench_hvr.json)
            step_ms = 21.9 if args.head == 'hvr' else 17.8
            ar['expected_share_of_train_step'] = dict(step_ms_one_gpu=step_ms, measured_allreduce_ms=ar['ms'],
                                                      share_if_not_overlapped=round(ar['ms'] / (step_ms + ar['ms']), 4),
                                                      est_ring_share=round(ar['est_ring_one_link_ms'] / (step_ms + ar['est_ring_one_link_ms']), 4))
            out['train_allreduce'] = ar
        if world == 1 and not args.no_graphs and args.inflight == 1 and out.get('graphed_stream'):
            # (after everything else: the child shares the GPU with nothing of this process that is still running)
            ss = stream_side_measurement(args.head)
            if ss is not None:
                ss.pop('metric', None)
                (ss.get('rpn_proposals_one_frame') or {}).pop('what', None)
                out['graphed_stream']['pipelined_window_cus'] = ss
        if world == 1 and not args.no_train_step:
            ts = train_step_side_measurement(args.head)
            if ts is not None:
                out['train_step'] = ts
        print(json.dumps(out, separators=(',', ':')))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
