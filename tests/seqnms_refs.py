"""Host restatements of the Seq-NMS read-out (numpy, no GPU) -- the specification of DESIGN.md ("Seq-NMS read-out") in float32 with
its arithmetic order.  The reference tree has no Seq-NMS, so these are what the device kernels (hvrnet_amd/csrc/seqnms.hip) are
pinned to:
  seq_nms_ref         the plain loop: a full dynamic programme in every round, no shortcuts.
  seq_nms_exhaustive  an independent path search for tiny inputs (every link chain enumerated); shares only the IoU helper.
  video / quantised_video / degenerate_video   seeded inputs of the tests.
"""
import itertools

import numpy as np

F32 = np.float32


def iou_plus1(a, b):
    """[n,4] x [m,4] -> [n,m] f32: box_iou_plus1 of hvrnet_amd/csrc/nms_dev.h (the arithmetic order of nms_cpu.cpp, +1 pixel
    convention; fmaxf / fminf drop a NaN operand as np.fmax / np.fmin do)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    one, zero = F32(1), F32(0)
    xx1, yy1 = np.fmax(a[:, None, 0], b[None, :, 0]), np.fmax(a[:, None, 1], b[None, :, 1])
    xx2, yy2 = np.fmin(a[:, None, 2], b[None, :, 2]), np.fmin(a[:, None, 3], b[None, :, 3])
    w, h = np.fmax(zero, (xx2 - xx1) + one), np.fmax(zero, (yy2 - yy1) + one)
    inter = w * h
    aa = ((a[:, 2] - a[:, 0]) + one) * ((a[:, 3] - a[:, 1]) + one)
    ab = ((b[:, 2] - b[:, 0]) + one) * ((b[:, 3] - b[:, 1]) + one)
    with np.errstate(all='ignore'):
        out = inter / ((aa[:, None] + ab[None, :]) - inter)
    assert out.dtype == F32
    return out


def _matrices(boxes, link_thr, nms_thr):
    Fn = boxes.shape[0]
    with np.errstate(invalid='ignore'):
        links = [iou_plus1(boxes[t], boxes[t + 1]) >= F32(link_thr) for t in range(Fn - 1)]
        ovl = [iou_plus1(boxes[t], boxes[t]) >= F32(nms_thr) for t in range(Fn)]
    return links, ovl


def _class_ref(s, score_thr, links, ovl, rescore, info):
    """One class: s [F,R] f32 -> (keep [F,R] bool, out [F,R] f32 rescored)."""
    Fn, R = s.shape
    with np.errstate(invalid='ignore'):
        alive = s > F32(score_thr)
    keep, out = np.zeros((Fn, R), bool), np.zeros((Fn, R), F32)
    rounds = 0
    while alive.any():
        rounds += 1
        assert rounds <= Fn * R
        best, nxt = np.zeros((Fn, R), F32), np.full((Fn, R), -1, np.int64)
        for t in range(Fn - 1, -1, -1):
            m, nx = np.zeros(R, F32), np.full(R, -1, np.int64)
            if t + 1 < Fn:
                cand = links[t] & alive[t + 1][None, :]
                vals = np.where(cand, best[t + 1][None, :], F32(-np.inf))
                nx = vals.argmax(1)                      # first occurrence: the lowest j attaining the max
                m = vals[np.arange(R), nx].astype(F32)
                none = ~cand.any(1)
                m[none], nx[none] = F32(0), -1
            best[t] = s[t] + m                           # one f32 add per frame
            nxt[t] = nx
        masked = np.where(alive, best, F32(-np.inf))
        rt, ri = np.unravel_index(int(masked.argmax()), masked.shape)   # largest sum, lowest t, then lowest i
        path, t, i = [], int(rt), int(ri)
        while i >= 0:
            path.append((t, i))
            i, t = int(nxt[t, i]), t + 1
        n = len(path)
        if rescore == 'avg':
            val = F32(best[rt, ri] / F32(n))              # one f32 division
        elif rescore == 'max':
            val = max(s[t, i] for t, i in path)
        else:
            raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
        for t, i in path:
            keep[t, i], out[t, i] = True, val
            alive[t] &= ~ovl[t][i]
            alive[t, i] = False                           # unconditionally: a degenerate box has IoU NaN with itself
        if info is not None:
            info['paths'] = info.get('paths', 0) + 1
            info['long_paths'] = info.get('long_paths', 0) + (n > 1)
    return keep, out


def _frame_lists(boxes, kept, max_num):
    """kept: per class (keep [F,R], out [F,R]) -> dets [F,max_num,5], labels [F,max_num] int64, n [F] int32: per frame the kept rows
    class-major, ascending row, rescored scores; cut to max_num by (score descending, list position ascending); zeros behind n."""
    Fn = boxes.shape[0]
    dets, labels, n = np.zeros((Fn, max_num, 5), F32), np.zeros((Fn, max_num), np.int64), np.zeros(Fn, np.int32)
    for t in range(Fn):
        rows = [(c, r) for c, (keep, _) in enumerate(kept) for r in np.flatnonzero(keep[t])]
        sc = np.array([kept[c][1][t, r] for c, r in rows], F32)
        order = np.arange(len(rows))
        if len(rows) > max_num:
            order = np.argsort(-sc, kind='stable')[:max_num]
        n[t] = len(order)
        for q, o in enumerate(order):
            c, r = rows[o]
            dets[t, q, :4], dets[t, q, 4], labels[t, q] = boxes[t, r], sc[o], c
    return dets, labels, n


def seq_nms_ref(boxes, scores, score_thr, link_thr=0.5, nms_thr=0.3, max_num=300, rescore='avg', info=None):
    """boxes [F,R,4], scores [F,R,ncls] -> (dets [F,max_num,5], labels [F,max_num] int64, n [F] int32)."""
    boxes, scores = np.ascontiguousarray(boxes, F32), np.ascontiguousarray(scores, F32)
    assert score_thr >= 0 and max_num > 0 and boxes.shape[:2] == scores.shape[:2]
    if rescore not in ('avg', 'max'):
        raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
    links, ovl = _matrices(boxes, link_thr, nms_thr)
    kept = [_class_ref(scores[:, :, c], score_thr, links, ovl, rescore, info) for c in range(1, scores.shape[2])]
    if info is not None:
        info['kept'] = kept
    return _frame_lists(boxes, kept, max_num)


# ---- independent search for tiny inputs ----
def _chains(alive, links, t, i):
    """every link chain over alive boxes that starts at (t, i), as tuples of rows (prefixes included)."""
    yield (i,)
    if t + 1 < len(alive):
        for j in sorted(alive[t + 1]):
            if links[t][i, j]:
                for rest in _chains(alive, links, t + 1, j):
                    yield (i,) + rest


def seq_nms_exhaustive(boxes, scores, score_thr, link_thr=0.5, nms_thr=0.3, max_num=300, rescore='avg'):
    """Same contract as seq_nms_ref on inputs whose sums are exact (scores k/64, integer corners): per class, among ALL link chains
    the largest sum, then the lowest root (t, i), then the lexicographically lowest successor rows."""
    from fractions import Fraction
    boxes, scores = np.ascontiguousarray(boxes, F32), np.ascontiguousarray(scores, F32)
    Fn, R, ncls = scores.shape
    iou_next = [iou_plus1(boxes[t], boxes[t + 1]) for t in range(Fn - 1)]
    iou_same = [iou_plus1(boxes[t], boxes[t]) for t in range(Fn)]
    with np.errstate(invalid='ignore'):
        links = [m >= F32(link_thr) for m in iou_next]
    kept = []
    for c in range(1, ncls):
        alive = [set(i for i in range(R) if scores[t, i, c] > F32(score_thr)) for t in range(Fn)]
        keep, out = np.zeros((Fn, R), bool), np.zeros((Fn, R), F32)
        while any(alive):
            found = None
            for t, i in itertools.product(range(Fn), range(R)):
                if i not in alive[t]:
                    continue
                for ch in _chains(alive, links, t, i):
                    total = sum(Fraction(float(scores[t + d, r, c])) for d, r in enumerate(ch))
                    rank = (-total, t, ch)                       # tuples compare lexicographically
                    if found is None or rank < found[0]:
                        found = (rank, t, ch, total)
            _, t0, ch, total = found
            assert F32(float(total)) == total, 'the exhaustive search is specified on exactly representable sums'
            val = F32(F32(float(total)) / F32(len(ch))) if rescore == 'avg' else max(scores[t0 + d, r, c] for d, r in enumerate(ch))
            for d, r in enumerate(ch):
                t = t0 + d
                keep[t, r], out[t, r] = True, val
                with np.errstate(invalid='ignore'):
                    alive[t] = set(i for i in alive[t] if i != r and not iou_same[t][r, i] >= F32(nms_thr))
        kept.append((keep, out))
    return _frame_lists(boxes, kept, max_num)


# ---- seeded inputs ----
def tiny_case(seed):
    """F, R in 1..4, two foreground classes, boxes drawn from a pool of five integer boxes (duplicates are common), scores k/64 from
    a short list (equal scores are common); some scores sit below the threshold 4/64."""
    rng = np.random.RandomState(seed)
    Fn, R = int(rng.randint(1, 5)), int(rng.randint(1, 5))
    pool = np.array([[0, 0, 9, 9], [0, 0, 9, 4], [2, 1, 11, 10], [20, 20, 29, 29], [0, 0, 9, 9]], F32)
    pool[4] += F32(rng.randint(0, 3))
    boxes = pool[rng.randint(0, len(pool), size=(Fn, R))]
    levels = np.array([1, 4, 16, 16, 32, 32, 48, 64], F32) / F32(64)
    scores = levels[rng.randint(0, len(levels), size=(Fn, R, 3))]
    return boxes, scores, 4.0 / 64.0


def video(seed, Fn, R, ncls, tracks=3, clutter=0.5, pad=2, low=0.02):
    """Tracks plus clutter: `tracks` objects drift through the frames, each with two jittered duplicates of lower score; a
    fraction `clutter` of the remaining rows are random boxes with one raised class score; the rest stay below `low`; the last
    `pad` rows are padding (all-zero scores).  Rows are permuted per frame.  -> boxes [F,R,4], scores [F,R,ncls] f32."""
    rng = np.random.RandomState(seed)
    boxes, scores = np.zeros((Fn, R, 4), F32), np.zeros((Fn, R, ncls), F32)
    pad = min(pad, max(R - 1, 0))
    live = R - pad
    start = rng.uniform(50, 500, size=(tracks, 2))
    vel = rng.uniform(-6, 6, size=(tracks, 2))
    size = rng.uniform(40, 160, size=(tracks, 2))
    cls = rng.randint(1, ncls, size=tracks)
    gone = [set(rng.choice(Fn, size=max(Fn // 6, 0), replace=False).tolist()) for _ in range(tracks)]   # frames a track is missed in
    for t in range(Fn):
        xy = rng.uniform(0, 800, size=(live, 2))
        wh = rng.uniform(10, 200, size=(live, 2))
        b = np.concatenate([xy, xy + wh], 1)
        s = rng.uniform(0, low, size=(live, ncls))
        is_clutter = rng.uniform(size=live) < clutter
        cc = rng.randint(1, ncls, size=live)
        s[np.flatnonzero(is_clutter), cc[is_clutter]] = rng.uniform(0, 0.6, size=int(is_clutter.sum()))
        row = 0
        for k in range(tracks):
            if t in gone[k]:
                continue
            base = np.concatenate([start[k] + vel[k] * t, start[k] + vel[k] * t + size[k]])
            for d in range(3):
                if row >= live:
                    break
                b[row] = base + (rng.uniform(-4, 4, size=4) if d else 0)
                s[row] = rng.uniform(0, low, size=ncls)
                s[row, cls[k]] = rng.uniform(0.5, 0.95) * (1.0 if d == 0 else 0.7)
                row += 1
        perm = rng.permutation(live)
        boxes[t, :live], scores[t, :live] = b[perm], s[perm]
    return boxes, scores


def quantised_video(seed, Fn, R, ncls):
    """Equal boxes and equal scores everywhere: integer boxes from a pool of twelve, scores from four dyadic levels."""
    rng = np.random.RandomState(seed)
    pool = np.array([[x, y, x + w, y + h] for x, y, w, h in
                     [(0, 0, 9, 9), (0, 0, 9, 4), (2, 1, 9, 9), (4, 4, 9, 9), (20, 20, 9, 9), (20, 22, 9, 9), (40, 0, 19, 9), (40, 0, 9, 9),
                      (45, 0, 9, 9), (0, 40, 9, 19), (0, 45, 9, 9), (3, 42, 9, 9)]], F32)
    boxes = pool[rng.randint(0, len(pool), size=(Fn, R))]
    levels = np.array([0, 0.25, 0.5, 0.5, 0.75], F32)
    scores = levels[rng.randint(0, len(levels), size=(Fn, R, ncls))]
    return boxes, scores


def degenerate_video():
    """Three frames of the same five rows: a normal box, an inverted box, a zero-area box (x2 = x1 - 1), a box with x2 < x1 - 1 whose
    +1 width is negative, and a zero-area box in both axes (IoU with itself 0 / 0 = NaN).  One foreground class, every row a candidate."""
    frame = np.array([[10, 10, 50, 50], [60, 60, 40, 40], [70, 10, 69, 30], [90, 10, 80, 30], [5, 5, 4, 4]], F32)
    boxes = np.stack([frame] * 3)
    scores = np.zeros((3, 5, 2), F32)
    scores[:, :, 1] = np.array([[0.9, 0.8, 0.7, 0.6, 0.5], [0.5, 0.6, 0.7, 0.8, 0.9], [0.3, 0.3, 0.3, 0.3, 0.3]], F32)
    return boxes, scores
