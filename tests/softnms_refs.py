"""numpy restatement of the reference's Soft-NMS (mmdet/ops/nms/src/soft_nms_cpu.pyx behind nms_wrapper.soft_nms) and of
multiclass_nms around it (mmdet/core/post_processing/bbox_nms.py:32-61 with nms_cfg type='soft_nms'), for the sizes and inputs no
fixture can hold.  tests/test_softnms_host.py pins it to the recorded outputs of the compiled reference bit for bit
(tests/golden/g20_soft_nms.npz: indices, score bits, order).

Round form.  State = (box, score, original index) rows in a physical order the algorithm permutes, N live rows.  Round i:
  1. winner = arg max of the scores at positions i .. N-1, lowest position on equal scores;
  2. rows i and winner change places;
  3. every row p in i+1 .. N-1 that overlaps row i (iw > 0 and ih > 0) is rescored, score *= weight, and is DEAD if the new
     score < min_score (a row that does not overlap is never tested).  The .pyx removes a dead row by moving row N-1 into its place
     and examining that place again; over the round that is: N' = N - #dead, the dead positions < N' in ascending order receive the
     live rows at positions >= N' in descending order.
Arithmetic = what the compiled .pyx does: its `cdef float` expressions contain the literal 1, a C double, so the +1 terms and the
area products are f64, every assignment to a `cdef float` rounds to f32 once, iw * ih and the quotient are f32, and the gaussian weight
is numpy's f64 exp of an f32 argument, rounded to f32."""
import numpy as np

f32, f64 = np.float32, np.float64
METHODS = {'linear': 1, 'gaussian': 2}


def ulp_distance(a, b):
    """Number of f32 values between a and b (same sign or zero)."""
    ia = np.asarray(a, f32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _weights(t, rows, iou_thr, method, sigma):
    """-> (overlaps [m] bool, weight [m] f32) of rows [m,>=4] against the winner t."""
    tx1, ty1, tx2, ty2 = t[0], t[1], t[2], t[3]
    x1, y1, x2, y2 = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    mn = lambda a, b: np.where(a <= b, a, b)     # noqa: E731  (soft_nms_cpu.pyx:15-19)
    mx = lambda a, b: np.where(a >= b, a, b)     # noqa: E731
    with np.errstate(all='ignore'):
        iw = ((mn(tx2, x2) - mx(tx1, x1)).astype(f64) + 1.0).astype(f32)
        ih = ((mn(ty2, y2) - mx(ty1, y1)).astype(f64) + 1.0).astype(f32)
        ovl = (iw > 0) & (ih > 0)
        area = (((x2 - x1).astype(f64) + 1.0) * ((y2 - y1).astype(f64) + 1.0)).astype(f32)
        inter = iw * ih
        tarea = (f64(tx2 - tx1) + 1.0) * (f64(ty2 - ty1) + 1.0)
        ua = (tarea + area.astype(f64) - inter.astype(f64)).astype(f32)
        ov = inter / ua
        if method == 1:
            w = np.where(ov > iou_thr, (1.0 - ov.astype(f64)).astype(f32), f32(1))
        else:
            w = np.exp(((-(ov * ov)) / sigma).astype(f64)).astype(f32)
    return ovl, w.astype(f32)


def soft_nms(dets, iou_thr, method='linear', sigma=0.5, min_score=1e-3, info=None):
    """dets [n,5] f32 -> (new_dets [k,5] with rescored scores, inds [k] int64) in selection order (nms_wrapper.py:64-102).
    info (a dict) receives: 'decays' [k] = rescorings each kept row received, 'rounds', 'min_gap_ulp' = the smallest non-zero f32
    distance between a round's winner and its runner-up, 'min_thr_ulp' = the smallest distance of a rescored score to min_score."""
    if method not in METHODS:
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    code = METHODS[method]
    b = np.array(dets, dtype=f32, copy=True).reshape(-1, 5)
    n = b.shape[0]
    inds = np.arange(n, dtype=np.int64)
    decays = np.zeros(n, np.int64)
    iou_thr, sigma, min_score = f32(iou_thr), f32(sigma), f32(min_score)
    N, i = n, 0
    gap, thr_gap = 1 << 40, 1 << 40
    while i < N:
        s = b[i:N, 4]
        w = i + int(np.argmax(s))                 # first maximum = lowest position
        if info is not None and N - i > 1:
            rest = np.delete(s, w - i)
            d = int(ulp_distance(s[w - i], rest.max())) if (s[w - i] >= 0) == (rest.max() >= 0) else 1 << 30
            if d > 0:
                gap = min(gap, d)
        if w != i:
            b[[i, w]] = b[[w, i]]
            inds[[i, w]] = inds[[w, i]]
            decays[[i, w]] = decays[[w, i]]
        if N - i > 1:
            ovl, wt = _weights(b[i], b[i + 1:N], iou_thr, code, sigma)
            new = (wt * b[i + 1:N, 4]).astype(f32)
            b[i + 1:N, 4] = np.where(ovl, new, b[i + 1:N, 4])
            decays[i + 1:N] += ovl
            if info is not None and ovl.any():
                same = ovl & (new > 0)
                if same.any() and min_score > 0:
                    thr_gap = min(thr_gap, int(ulp_distance(new[same], min_score).min()))
            dead = ovl & (new < min_score)
            D = int(dead.sum())
            if D:
                pos = np.arange(i + 1, N)
                Nn = N - D
                holes = pos[dead & (pos < Nn)]
                srcs = pos[~dead & (pos >= Nn)][::-1]
                b[holes] = b[srcs]
                inds[holes] = inds[srcs]
                decays[holes] = decays[srcs]
                N = Nn
        i += 1
    if info is not None:
        info.update(decays=decays[:N].copy(), rounds=N, min_gap_ulp=gap, min_thr_ulp=thr_gap)
    return b[:N].copy(), inds[:N].copy()


def multiclass(boxes, scores, score_thr, nms_cfg, max_num=-1, info=None):
    """bbox_nms.py:35-61 for class-agnostic boxes [R,4] and scores [R,ncls] (numpy) -> (dets [k,5], labels [k] int64).  The max_num
    cut orders by (rescored score descending, position in the class-major list ascending).  info receives 'decays' [k], 'rows' [k]
    (input row of each detection), 'per_class' = [(candidates, survivors)] and 'cut_ties' = whether two equal scores met in the sort."""
    cfg = dict(nms_cfg)
    assert cfg.pop('type', 'soft_nms') == 'soft_nms'
    boxes, scores = np.asarray(boxes, f32), np.asarray(scores, f32)
    out_d, out_l, out_k, out_r, per = [], [], [], [], []
    for c in range(1, scores.shape[1]):
        sel = np.nonzero(scores[:, c] > f32(score_thr))[0]
        if sel.size == 0:
            per.append((0, 0))
            continue
        sub = {}
        d, ind = soft_nms(np.concatenate([boxes[sel], scores[sel, c:c + 1]], 1), info=sub, **cfg)
        out_d.append(d)
        out_l.append(np.full(d.shape[0], c - 1, np.int64))
        out_k.append(sub['decays'])
        out_r.append(sel[ind])
        per.append((int(sel.size), int(d.shape[0])))
    if not out_d:
        if info is not None:
            info.update(decays=np.zeros(0, np.int64), rows=np.zeros(0, np.int64), per_class=per, cut_ties=False)
        return np.zeros((0, 5), f32), np.zeros(0, np.int64)
    d, l, k, r = np.concatenate(out_d), np.concatenate(out_l), np.concatenate(out_k), np.concatenate(out_r)
    ties = False
    if d.shape[0] > max_num:
        order = np.argsort(-d[:, 4].astype(f64), kind='stable')
        ties = bool(np.unique(d[:, 4]).size < d.shape[0])
        order = order[:max_num]
        d, l, k, r = d[order], l[order], k[order], r[order]
    if info is not None:
        info.update(decays=k, rows=r, per_class=per, cut_ties=ties)
    return d, l


def clustered_dets(seed, n, quantised=False, extent=(600., 1000.)):
    """A random list of n boxes in a few clusters (the shape of an RCNN read-out): [n,5] f32.  quantised: boxes duplicated and scores
    rounded to 0.1, so that exact ties abound."""
    rng = np.random.RandomState(seed)
    k = max(1, n // 12)
    cx, cy = rng.uniform(80, extent[1] - 80, k), rng.uniform(60, extent[0] - 60, k)
    w, h = rng.uniform(40, 260, k), rng.uniform(40, 220, k)
    a = rng.randint(0, k, n)
    x = cx[a] + rng.normal(0, 0.12, n) * w[a]
    y = cy[a] + rng.normal(0, 0.12, n) * h[a]
    ww, hh = w[a] * np.exp(rng.normal(0, 0.2, n)), h[a] * np.exp(rng.normal(0, 0.2, n))
    b = np.stack([np.clip(x - ww / 2, 0, extent[1] - 2), np.clip(y - hh / 2, 0, extent[0] - 2),
                  np.clip(x + ww / 2, 1, extent[1] - 1), np.clip(y + hh / 2, 1, extent[0] - 1)], 1)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
    s = rng.uniform(0.02, 1.0, n)
    if quantised:
        dup = rng.randint(0, n, n)
        take = rng.uniform(size=n) < 0.4
        b[take] = b[dup[take]]
        b = np.round(b)
        s = np.maximum(np.round(s, 1), 0.1)
    return np.concatenate([b, s[:, None]], 1).astype(f32)


def class_scores(seed, R, ncls, sharp=4.0):
    """Softmax-like score rows [R, ncls] f32 (column 0 = background)."""
    rng = np.random.RandomState(seed)
    z = rng.normal(0, sharp, (R, ncls))
    z -= z.max(1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(1, keepdims=True)).astype(f32)


def score_tolerance(want_scores, decays, method):
    """The allowed |got - want| per detection: linear is bit-exact; gaussian one f32 ulp per rescoring the entry received (each
    weight is one correctly rounded f32 of an f64 exp whose last bit may differ between the device's libm and numpy's)."""
    want_scores = np.asarray(want_scores, f32)
    if method != 'gaussian':
        return np.zeros(want_scores.shape, f64)
    return decays.astype(f64) * np.spacing(np.abs(want_scores)).astype(f64)
