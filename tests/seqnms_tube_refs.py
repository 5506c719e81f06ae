"""Host restatement of the batched Seq-NMS read-out with tube outputs (numpy, no GPU) -- DESIGN.md 8d (the per-problem algorithm,
restated here as a plain loop of its own) and 8e (problems and tubes).  The device (hvrnet_amd/csrc/seqnms.hip through
native.seq_nms_batched) is pinned to seq_nms_tubes_ref on all seven outputs, bit for bit.
  seq_nms_tubes_ref         the plain loop per problem and class; records every selected path.
  exhaustive_chains         tests/seqnms_refs.py's exhaustive search on one problem, recording the chains it selects.
  tubes_of                  the tube table of one problem from recorded paths.
Only iou_plus1 and the seeded inputs come from tests/seqnms_refs.py (unchanged)."""
import itertools

import numpy as np

from tests.seqnms_refs import iou_plus1

F32 = np.float32


def _class_paths(s, score_thr, links, ovl, rescore):
    """One class of one problem: s [F,R] -> the selected paths in selection order, each (root frame, [rows], rescored value)."""
    Fn, R = s.shape
    with np.errstate(invalid='ignore'):
        alive = s > F32(score_thr)                       # a NaN score is no candidate
    paths = []
    while alive.any():
        assert len(paths) <= Fn * R
        best, nxt = np.zeros((Fn, R), F32), np.full((Fn, R), -1, np.int64)
        for t in range(Fn - 1, -1, -1):                  # backward in time; the problem's last frame has no links
            m, nx = np.zeros(R, F32), np.full(R, -1, np.int64)
            if t + 1 < Fn:
                cand = links[t] & alive[t + 1][None, :]
                vals = np.where(cand, best[t + 1][None, :], F32(-np.inf))
                nx = vals.argmax(1)                      # the first occurrence: the lowest j attaining the max
                m = vals[np.arange(R), nx].astype(F32)
                none = ~cand.any(1)
                m[none], nx[none] = F32(0), -1
            best[t], nxt[t] = s[t] + m, nx               # one f32 add per frame
        masked = np.where(alive, best, F32(-np.inf))
        root = tuple(int(x) for x in np.unravel_index(int(masked.argmax()), masked.shape))   # the largest sum; the lowest t, then the lowest i
        t, i = root
        rows = []
        while i >= 0:
            rows.append(int(i))
            i, t = int(nxt[t, i]), t + 1
        n = len(rows)
        if rescore == 'avg':
            val = F32(best[root] / F32(n))               # one f32 division
        elif rescore == 'max':
            val = max(s[root[0] + d, r] for d, r in enumerate(rows))
        else:
            raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
        for d, r in enumerate(rows):
            t = root[0] + d
            alive[t] &= ~ovl[t][r]                       # the overlaps of the path box, at nms_thr
            alive[t, r] = False                          # and the path box itself, unconditionally (IoU with itself may be NaN)
        paths.append((int(root[0]), rows, F32(val)))
    return paths


def tubes_of(problem, paths_by_class):
    """paths_by_class[c] = [(root frame, rows, value)] in selection order -> (table [n,4] int32, scores [n] f32, id of every kept
    (class, frame, row)): ids class-major, within a class in selection order; length = the boxes selected on the path."""
    table, vals, ids = [], [], {}
    for c, paths in enumerate(paths_by_class):
        for t0, rows, val in paths:
            for d, r in enumerate(rows):
                assert (c, t0 + d, r) not in ids
                ids[(c, t0 + d, r)] = len(table)
            table.append((problem, c, t0, len(rows)))
            vals.append(val)
    return np.array(table, np.int32).reshape(-1, 4), np.array(vals, F32), ids


def _frame_rows(boxes, paths_by_class, ids, max_num):
    """The per-frame lists of one problem (8d step 4) + the tube id of every output row (-1 behind n)."""
    Fn = boxes.shape[0]
    dets, labels = np.zeros((Fn, max_num, 5), F32), np.zeros((Fn, max_num), np.int64)
    n, tube_ids = np.zeros(Fn, np.int32), np.full((Fn, max_num), -1, np.int32)
    score = {}
    for c, paths in enumerate(paths_by_class):
        for t0, rows, val in paths:
            for d, r in enumerate(rows):
                score[(c, t0 + d, r)] = val
    for t in range(Fn):
        rows = sorted((c, r) for c, tt, r in score if tt == t)          # class-major, ascending row
        sc = np.array([score[(c, t, r)] for c, r in rows], F32)
        order = np.arange(len(rows))
        if len(rows) > max_num:
            order = np.argsort(-sc, kind='stable')[:max_num]            # score descending, list position ascending
        n[t] = len(order)
        for q, o in enumerate(order):
            c, r = rows[o]
            dets[t, q, :4], dets[t, q, 4], labels[t, q], tube_ids[t, q] = boxes[t, r], sc[o], c, ids[(c, t, r)]
    return dets, labels, n, tube_ids


def seq_nms_tubes_ref(boxes, scores, frame_counts, score_thr, link_thr=0.5, nms_thr=0.3, max_num=300, rescore='avg', max_tubes=None,
                      fill=None, info=None):
    """boxes [Ftot,R,4], scores [Ftot,R,ncls], frame_counts: P counts >= 1 summing to Ftot -> the seven outputs (dets, labels, n,
    tube_ids, tubes [max_tubes,4], tube_scores [max_tubes], tube_start [P+1]).  max_tubes defaults to the true total; rows at and
    behind min(total, max_tubes) keep `fill` = (table value, score value) (default zeros): the device does not touch them."""
    boxes, scores = np.ascontiguousarray(boxes, F32), np.ascontiguousarray(scores, F32)
    counts = [int(c) for c in frame_counts]
    assert score_thr >= 0 and max_num > 0 and boxes.shape[:2] == scores.shape[:2] and min(counts) >= 1 and sum(counts) == boxes.shape[0]
    if rescore not in ('avg', 'max'):
        raise ValueError('Invalid rescore for Seq-NMS: {} (avg, max)'.format(rescore))
    outs, tables, vals, start, f0 = [], [], [], [0], 0
    for p, Fn in enumerate(counts):
        b, s = boxes[f0:f0 + Fn], scores[f0:f0 + Fn]                    # nothing crosses a problem boundary
        with np.errstate(invalid='ignore'):
            links = [iou_plus1(b[t], b[t + 1]) >= F32(link_thr) for t in range(Fn - 1)]
            ovl = [iou_plus1(b[t], b[t]) >= F32(nms_thr) for t in range(Fn)]
        paths = [_class_paths(s[:, :, c], score_thr, links, ovl, rescore) for c in range(1, s.shape[2])]
        table, val, ids = tubes_of(p, paths)
        outs.append(_frame_rows(b, paths, ids, max_num))
        tables.append(table)
        vals.append(val)
        start.append(start[-1] + len(table))
        f0 += Fn
        if info is not None:
            info.setdefault('paths', []).append(paths)
    dets, labels, n, tube_ids = [np.concatenate([o[k] for o in outs]) for k in range(4)]
    total = start[-1]
    cap = total if max_tubes is None else int(max_tubes)
    fill = (0, 0) if fill is None else fill
    tubes, tube_scores = np.full((cap, 4), fill[0], np.int32), np.full(cap, fill[1], F32)
    k = min(total, cap)
    tubes[:k], tube_scores[:k] = np.concatenate(tables)[:k], np.concatenate(vals)[:k]
    return dets, labels, n, tube_ids, tubes, tube_scores, np.array(start, np.int32)


# ---- the exhaustive search of tests/seqnms_refs.py, recording its chains ----
def _chains(alive, links, t, i):
    yield (i,)
    if t + 1 < len(alive):
        for j in sorted(alive[t + 1]):
            if links[t][i, j]:
                for rest in _chains(alive, links, t + 1, j):
                    yield (i,) + rest


def exhaustive_chains(boxes, scores, score_thr, link_thr=0.5, nms_thr=0.3, rescore='avg'):
    """One problem whose sums are exact (scores k/64, integer corners): per class the chains an exhaustive search over ALL link
    chains selects -- the largest sum, then the lowest root (t, i), then the lexicographically lowest successor rows -- as
    [(root frame, rows, value)] in selection order.  Shares only iou_plus1 with the plain loop above."""
    from fractions import Fraction
    boxes, scores = np.ascontiguousarray(boxes, F32), np.ascontiguousarray(scores, F32)
    Fn, R, ncls = scores.shape
    iou_next = [iou_plus1(boxes[t], boxes[t + 1]) for t in range(Fn - 1)]
    iou_same = [iou_plus1(boxes[t], boxes[t]) for t in range(Fn)]
    with np.errstate(invalid='ignore'):
        links = [m >= F32(link_thr) for m in iou_next]
    out = []
    for c in range(1, ncls):
        alive = [set(i for i in range(R) if scores[t, i, c] > F32(score_thr)) for t in range(Fn)]
        paths = []
        while any(alive):
            found = None
            for t, i in itertools.product(range(Fn), range(R)):
                if i not in alive[t]:
                    continue
                for ch in _chains(alive, links, t, i):
                    total = sum(Fraction(float(scores[t + d, r, c])) for d, r in enumerate(ch))
                    rank = (-total, t, ch)
                    if found is None or rank < found[0]:
                        found = (rank, t, ch, total)
            _, t0, ch, total = found
            assert F32(float(total)) == total
            val = F32(F32(float(total)) / F32(len(ch))) if rescore == 'avg' else max(scores[t0 + d, r, c] for d, r in enumerate(ch))
            for d, r in enumerate(ch):
                t = t0 + d
                with np.errstate(invalid='ignore'):
                    alive[t] = set(i for i in alive[t] if i != r and not iou_same[t][r, i] >= F32(nms_thr))
            paths.append((t0, [int(r) for r in ch], F32(val)))
        out.append(paths)
    return out
