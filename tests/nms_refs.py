"""Host statements (numpy) of the greedy NMS read-out kernels of hvrnet_amd/csrc/nms.hip -- hvr_nms, hvr_nms_first, hvr_multiclass_nms -- the
input families on which the statements are exact, and the cases the GPU test (tests/test_nms_kernels_gpu.py) runs.  Reads nothing
outside tests/.  tests/test_nms_refs.py pins the statements to the recorded vectors (g3_nms, g8_det), checks that every case exercises
what it is listed for (the `info` dicts) and that every planted mistake that applies to a case changes its answer; it is also what
fixed the seeds below (first of 1, 2, 3, ... that meets the case's conditions).

Exactness.  The main families have INTEGER box coordinates below 2^12, so every width, height, area, intersection and union is an
integer below 2^24, an exact f32 whatever the compiler contracts, and the one rounding -- the f32 division inter / union -- is the
same correctly rounded quotient on the host and on the device.  The verdict `ovr >= thr` needs no tolerance.  Such boxes put many
IoUs exactly on 1/2, 1/3, 2/3 ... (the trick of test_nms_first_on_boxes_whose_ious_sit_on_the_threshold).  Scores come from a
dyadic grid k / G, k >= 1, so equal scores are common; no score is a zero, of either sign: float_key orders -0.0 behind +0.0 while the
tie rule below treats equal floats alike (nms.hip's header says so), and the pair is kept out of the families.

Tie rule (top of nms.hip): higher score first, lower input index first on equal scores."""
import functools

import numpy as np

f32 = np.float32
ONE = f32(1)

MISTAKES_NMS = ('gt', 'no_plus1', 'tie_high_index', 'keep_score_order')
MISTAKES_MC = MISTAKES_NMS + ('unstable_cut', 'cut_before_sort', 'score_ge_thr')


# ------------------------------------------------------------------------------------------------ statements
def _area(b, plus1):
    one = ONE if plus1 else f32(0)
    return (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)


def iou_rows(a, a_area, rest, rest_area, plus1=True):
    """box_iou_plus1 (nms_dev.h; nms_cpu.cpp:18,46-54) of ONE box `a` [4] (the earlier box: its area comes first in the union)
    against rest [m,4], f32 step by step in the kernel's order.  0 / 0 -> NaN, x / 0 -> inf, as the f32 expression gives."""
    one = ONE if plus1 else f32(0)
    with np.errstate(all='ignore'):
        w = np.maximum(f32(0), np.minimum(a[2], rest[:, 2]) - np.maximum(a[0], rest[:, 0]) + one)
        h = np.maximum(f32(0), np.minimum(a[3], rest[:, 3]) - np.maximum(a[1], rest[:, 1]) + one)
        inter = w * h
        return inter / (a_area + rest_area - inter)


def visiting_order(scores, mistake=None):
    """positions -> input index: score descending, lower index first on equal scores (a stable sort of the negated scores)."""
    s = np.asarray(scores, f32)
    if mistake == 'tie_high_index':
        return (len(s) - 1 - np.argsort(-s[::-1], kind='stable')).astype(np.int64)
    return np.argsort(-s, kind='stable').astype(np.int64)


def greedy_sweep(dets, thr, ge=True, mistake=None, info=None):
    """The whole greedy loop without a cap -> (survivors as input indices in VISITING order, their positions in score order).
    Row by row: one survivor against the boxes still alive behind it; no n x n matrix."""
    d = np.ascontiguousarray(np.asarray(dets, f32).reshape(-1, 5))
    n = d.shape[0]
    thr = f32(thr)
    if mistake == 'gt':
        ge = False
    plus1 = mistake != 'no_plus1'
    order = visiting_order(d[:, 4], mistake)
    b = d[order, :4]
    area = _area(b, plus1)
    pos = np.arange(n, dtype=np.int64)          # positions (score order) still alive, ascending
    kept = []
    exact = 0
    cross = False
    while pos.size:
        p = int(pos[0])
        kept.append(p)
        rest = pos[1:]
        if rest.size == 0:
            break
        ovr = iou_rows(b[p], area[p], b[rest], area[rest], plus1)
        with np.errstate(invalid='ignore'):
            hit = (ovr >= thr) if ge else (ovr > thr)
            exact += int((ovr == thr).sum())
        if p < 4096 and not cross and bool((hit & (rest >= 4096)).any()):
            cross = True
        pos = rest[~hit]
    kept = np.asarray(kept, dtype=np.int64)
    if info is not None:
        s = d[order, 4]
        info.update(n=n, survivors=int(kept.size), adjacent_ties=int((s[1:] == s[:-1]).sum()), exact_hits=exact,
                    last_survivor_pos=int(kept[-1]) if kept.size else -1, cross_half=cross)
    return order[kept], kept


def cut_sweep(sweep, max_keep=0, mistake=None, info=None):
    """The first max_keep survivors (all when max_keep <= 0) of a greedy_sweep result as ascending input indices: the contract of
    `keep` (nms_cpu.cpp:58; rpn_head.py:95-97 for the cap)."""
    idx, pos = sweep
    if info is not None:
        reached = 0 < max_keep <= len(idx)
        info.update(cap_reached=reached, cap_chunk=int(pos[max_keep - 1]) // 64 if reached else -1)
    if max_keep > 0:
        idx = idx[:max_keep]
    return [int(i) for i in idx] if mistake == 'keep_score_order' else sorted(int(i) for i in idx)


def greedy_nms(dets, thr, ge=True, max_keep=0, mistake=None, info=None):
    """hvr_nms (max_keep = 0) / hvr_nms_first: candidates visited by score descending, lower index first on equal scores; IoU with
    the "+1" convention in box_iou_plus1's order; a candidate is suppressed by an earlier survivor when ovr >= thr (ge) or ovr > thr;
    with max_keep > 0 the loop stops after max_keep survivors (what lies behind is never looked at, and the outcome is the same as
    cutting the full sweep).  -> ascending input indices.
    info: n, survivors (of the uncapped sweep), adjacent_ties (equal-score pairs adjacent in visiting order), exact_hits (evaluated
    pairs with IoU == thr), last_survivor_pos (score position), cross_half (a survivor at position < 4096 suppressed a box at position
    >= 4096), cap_reached, cap_chunk (64-box chunk of the max_keep-th survivor).
    mistake: 'gt' (> where >= is meant), 'no_plus1', 'tie_high_index' (equal scores: highest index first), 'keep_score_order'
    (survivors returned in score order)."""
    return cut_sweep(greedy_sweep(dets, thr, ge, mistake, info), max_keep, mistake, info)


def multiclass_list(boxes, scores, score_thr, iou_thr, mistake=None, info=None):
    """bbox_nms.py:20-52 for class-agnostic boxes: per foreground class c (column c of scores) the rows with score > score_thr go
    through greedy NMS (>=); survivors concatenated class-major, roi ascending -> (rows [t], classes [t] 0-based, scores [t])."""
    bx = np.asarray(boxes, f32).reshape(-1, 4)
    sc = np.asarray(scores, f32)
    R, ncls = sc.shape
    st = f32(score_thr)
    rows, cls, ncand, nsurv, exact = [], [], [], [], 0
    for c in range(1, ncls):
        cand = np.nonzero(sc[:, c] >= st if mistake == 'score_ge_thr' else sc[:, c] > st)[0]
        ncand.append(int(cand.size))
        if cand.size == 0:
            nsurv.append(0)
            continue
        di = {}
        keep = greedy_nms(np.concatenate([bx[cand], sc[cand, c:c + 1]], 1), iou_thr, True, 0,
                          mistake if mistake in MISTAKES_NMS else None, di)
        exact += di['exact_hits']
        nsurv.append(len(keep))
        rows.extend(int(cand[k]) for k in keep)
        cls.extend([c - 1] * len(keep))
    rows, cls = np.asarray(rows, np.int64), np.asarray(cls, np.int64)
    s = sc[rows, cls + 1] if rows.size else np.zeros(0, f32)
    if info is not None:
        info.update(candidates=ncand, survivors=nsurv, total=int(rows.size), exact_hits=exact,
                    scores_on_thr=int((sc[:, 1:] == st).sum()))
    return rows, cls, s


def cut_list(boxes, lst, max_num, mistake=None, info=None):
    """bbox_nms.py:54-61: more than max_num survivors -> the max_num best by (score descending, list position ascending).
    max_num < 0 is the reference's default read literally (bbox_nms.py:55-59): `count > max_num` always holds, the list is sorted and
    `inds[:max_num]` drops its last |max_num| entries.  -> (dets [k,5] f32, labels [k] int64)."""
    rows, cls, s = lst
    t = rows.size
    sel = np.arange(t)
    if t > max_num:
        k = max_num if max_num >= 0 else max(t + max_num, 0)
        if mistake == 'cut_before_sort':
            sel = sel[:k]
            sel = sel[np.argsort(-s[sel], kind='stable')]
        elif mistake == 'unstable_cut':
            sel = (t - 1 - np.argsort(-s[::-1], kind='stable'))[:k]
        else:
            sel = np.argsort(-s, kind='stable')[:k]
        if info is not None:
            full = np.argsort(-s, kind='stable')
            info.update(cut=True, cut_tie=bool(0 < k < t and s[full[k - 1]] == s[full[k]]))
    elif info is not None:
        info.update(cut=False, cut_tie=False)
    bx = np.asarray(boxes, f32).reshape(-1, 4)
    dets = np.concatenate([bx[rows[sel]], s[sel, None]], 1).astype(f32).reshape(-1, 5)
    return dets, cls[sel].astype(np.int64)


def multiclass_nms(boxes, scores, score_thr, iou_thr, max_num, mistake=None, info=None):
    """hvr_multiclass_nms: multiclass_list, then cut_list.  info: per-class candidates / survivors, total, exact_hits, scores_on_thr
    (foreground scores equal to score_thr: strict >), cut, cut_tie (the last score taken equals the first one left out), max_num.
    mistake: the four of greedy_nms, 'unstable_cut' (ties at the cut taken from the end of the list), 'cut_before_sort' (the first
    max_num in class order), 'score_ge_thr' (>= on score_thr)."""
    out = cut_list(boxes, multiclass_list(boxes, scores, score_thr, iou_thr, mistake, info), max_num, mistake, info)
    if info is not None:
        info['max_num'] = max_num
    return out


# ------------------------------------------------------------------------------------------------ input families
G_SCORE = 256       # score grid of dense / sparse / degenerate: k / 256
CELL = 16           # lattice pitch of the sparse layouts; boxes of at most 12 x 12 inside a cell never reach a neighbour
SIZES = np.array([2, 3, 4, 6, 8, 12])


def _lattice(rng, n, ncell):
    """n boxes, each inside one of ncell 16-pixel lattice cells drawn with replacement (boxes of one cell overlap, others never);
    sides from SIZES, corners on a 4-pixel sub-grid: IoUs of 1/2, 1/3, 2/3, 1/4 ... are frequent."""
    cell = rng.integers(0, ncell, n)
    cols = 128
    x1 = (cell % cols) * CELL + rng.integers(0, 2, n) * 4
    y1 = (cell // cols) * CELL + rng.integers(0, 2, n) * 4
    w, h = SIZES[rng.integers(0, 4, n)], SIZES[rng.integers(0, 4, n)]     # sides <= 6 + offset 4: inside the cell
    return np.stack([x1, y1, x1 + w - 1, y1 + h - 1], 1).astype(f32)


def family(name, n, seed):
    """-> dets [n,5] f32.
    dense:      a small span, most boxes suppressed; one box in 32 is a straggler -- alone in a lattice cell far away, scores from the
                lowest eighth of the grid -- so the sweep walks to the end and still finds survivors there;
    sparse:     lattice cells drawn with replacement from as many cells as boxes: boxes that share a cell overlap, nine in ten survive;
    ties:       n // 8 + 2 distinct boxes (sparse layout), 8 distinct scores;
    degenerate: a wider dense layout with one box in four empty (x2 = x1 - 1: width 0, union may be 0, 0 / 0) and one in four inverted
                (x2 < x1 - 1 or y2 < y1 - 1: negative area); the verdict is what the f32 expression gives;
    float:      float coordinates in the style of test_kernels_gpu._boxes, distinct random scores."""
    rng = np.random.default_rng([seed, n, sorted(FAMILIES).index(name)])
    if name == 'float':
        span = 200.0 if n < 2000 else 900.0
        xy = rng.random((n, 2), dtype=f32) * f32(span)
        wh = rng.random((n, 2), dtype=f32) * f32(60) + f32(4)
        return np.concatenate([xy, xy + wh, rng.random((n, 1), dtype=f32)], 1).astype(f32)
    if name in ('dense', 'degenerate'):
        span = 3 + int(np.sqrt(n) / 8) if name == 'dense' else 6 + int(np.sqrt(n) / 3)
        xy = rng.integers(0, span, (n, 2))
        wh = rng.integers(4 if name == 'dense' else 1, 13, (n, 2))
        b = np.concatenate([xy, xy + wh - 1], 1).astype(f32)
        s = rng.integers(G_SCORE // 8, G_SCORE + 1, n)
        if name == 'dense':
            lone = rng.random(n) < 1.0 / 32
            far = _lattice(rng, n, 8192)
            far[:, [0, 2]] += 1024
            b[lone] = far[lone]
            s[lone] = rng.integers(1, G_SCORE // 8, int(lone.sum()))
        else:
            kind = rng.integers(0, 4, n)
            ax = rng.integers(0, 2, n)                   # which axis degenerates
            rows = np.arange(n)
            empty, inv = kind == 0, kind == 1
            b[rows[empty], 2 + ax[empty]] = b[rows[empty], ax[empty]] - 1
            b[rows[inv], 2 + ax[inv]] = b[rows[inv], ax[inv]] - 1 - rng.integers(1, 6, int(inv.sum()))
        return np.concatenate([b, (s / G_SCORE)[:, None]], 1).astype(f32)
    if name == 'sparse':
        b = _lattice(rng, n, max(n, 2))
        s = rng.integers(1, G_SCORE + 1, n)
        return np.concatenate([b, (s / G_SCORE)[:, None]], 1).astype(f32)
    if name == 'ties':
        m = n // 8 + 2
        proto = _lattice(rng, m, m)
        b = proto[rng.integers(0, m, n)]
        s = rng.integers(1, 9, n)
        return np.concatenate([b, (s / 8.0)[:, None]], 1).astype(f32)
    raise KeyError(name)


FAMILIES = ('dense', 'sparse', 'ties', 'degenerate', 'float')
THIRD = 1.0 / 3.0


def max_area(dets):
    d = np.asarray(dets, np.float64)
    return float(np.abs((d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)).max())


def float_margin(dets, thr):
    """min over all pairs of |IoU - thr| / thr with the IoU in f64 (row by row)."""
    d = np.asarray(dets, np.float64)
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    worst = np.inf
    for i in range(len(d) - 1):
        r = d[i + 1:]
        w = np.maximum(0, np.minimum(d[i, 2], r[:, 2]) - np.maximum(d[i, 0], r[:, 0]) + 1)
        h = np.maximum(0, np.minimum(d[i, 3], r[:, 3]) - np.maximum(d[i, 1], r[:, 1]) + 1)
        inter = w * h
        worst = min(worst, float(np.abs(inter / (area[i] + area[i + 1:] - inter) - thr).min()))
    return worst / thr


# ------------------------------------------------------------------------------------------------ cases of hvr_nms / hvr_nms_first
NMS_SIZES = (2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)     # (n = 1: the GPU file's own one-box test)
EDGE_SIZES = (65, 1025, 4097, 8192)
FIRST_KEEPS = (1, 64, 1023, 1024, 1025, 2048, 'n')
FLOAT_MARGIN = 2.0 ** -20     # relative distance every pair's f64 IoU keeps from thr in the float family
FLOAT_SIZES = (65, 700)     # sizes at which test_kernels_gpu.py already compares the device with the f32 step-by-step evaluation


def thr_of(fam, n):
    """dense / sparse alternate between the two thresholds with exact hits; the others stay on 1/2."""
    if fam in ('dense', 'sparse'):
        return 0.5 if NMS_SIZES.index(n) % 2 == 0 else THIRD
    return 0.5


# (family, n, thr, ge): every call of hvr_nms the GPU test makes
NMS_CASES = [(fam, n, thr_of(fam, n), ge) for fam in ('dense', 'sparse') for n in NMS_SIZES for ge in (True, False)] + \
            [(fam, n, 0.5, ge) for fam in ('ties', 'degenerate') for n in EDGE_SIZES for ge in (True, False)] + \
            [('float', n, 0.5, True) for n in FLOAT_SIZES]
# (family, n, thr, max_keep): every call of hvr_nms_first (ge); max_keep <= 1024 is the greedy kernel, above it mask + capped sweep
# ('n': max_keep = n; 's': max_keep = the survivor count, in the families whose last box survives -- the cap is reached in the last,
# ragged chunk: first_keep resolves both)
FIRST_CASES = [(fam, n, thr_of(fam, n) if n in NMS_SIZES else 0.5, k) for fam in ('dense', 'sparse', 'ties', 'degenerate')
               for n in EDGE_SIZES for k in FIRST_KEEPS + (('s',) if fam in ('dense', 'degenerate') and n % 64 else ())]


def nms_conditions(fam, n, thr, ge, info):
    """What makes the hvr_nms case (fam, n, thr, ge) worth running -> list of (name, holds).  A survivor count below n / 4 needs
    n >= 8 to be possible at all; at n = 2 `dense` means a pair whose IoU is exactly thr and `sparse` that both survive, the better
    one second."""
    c = []
    k = info['survivors']
    if fam == 'dense':
        if n >= 8:
            c.append(('keeps < n/4', k < n / 4))
        else:   # two boxes whose IoU is exactly thr: >= suppresses the second, > lets it live
            c.append(('the pair sits on thr', info['exact_hits'] == 1 and k == (1 if ge else 2)))
    if fam == 'sparse':
        c.append(('keeps > n/2', k > n / 2))
    if fam in ('dense', 'sparse') and n >= 63:
        c.append(('IoUs exactly on thr', info['exact_hits'] > 0))
        c.append(('adjacent equal scores', info['adjacent_ties'] > 0))
    if fam == 'ties':
        c.append(('adjacent equal scores', info['adjacent_ties'] > n // 2))
    if n == 4097:
        # one box only lies behind position 4095: it either survives (the sweep reads word 64 of the suppression set and finds its
        # bit clear) or was suppressed from the first half (finds it set).  AT_4097 says which reading each family takes; both occur.
        want = AT_4097[fam]
        c.append((want, info['last_survivor_pos'] >= 4096 if want == 'last survivor at position 4096' else info['cross_half']))
    if n > 4097:
        c.append(('last survivor at a position >= 4096', info['last_survivor_pos'] >= 4096))
        c.append(('cross-half suppression', info['cross_half']))
    return c


AT_4097 = {'dense': 'last survivor at position 4096', 'degenerate': 'last survivor at position 4096',
           'sparse': 'cross-half suppression', 'ties': 'cross-half suppression'}


def nms_mistakes(fam, n, thr, ge):
    """The planted mistakes that apply to the case: 'gt' where >= is meant and the family has IoUs on the threshold; 'no_plus1'
    everywhere; the tie rule where equal scores are the point; the output order wherever two boxes can survive."""
    m = ['no_plus1', 'keep_score_order']
    if ge and fam in ('dense', 'sparse', 'ties') and n >= 63:
        m.append('gt')
    if fam == 'ties':
        m.append('tie_high_index')
    if n == 2:
        m = ['keep_score_order'] if fam == 'sparse' else (['gt'] if ge else [])
    return m


# seeds per (family, n): the first of 1, 2, 3, ... for which every case of that (family, n) meets nms_conditions and is moved by
# every mistake of nms_mistakes / first_mistakes: `qualifies` below (tests/test_nms_refs.py::test_seeds_are_the_first_that_qualify)
SEEDS = {('dense', 2): 3, ('dense', 63): 2, ('dense', 64): 4, ('sparse', 2): 3, ('sparse', 64): 2, ('sparse', 65): 2, ('sparse', 4097): 3,
         ('ties', 65): 9}


def seed_of(fam, n):
    return SEEDS.get((fam, n), 1)


@functools.lru_cache(maxsize=None)
def seeded_dets(fam, n, seed):
    d = family(fam, n, seed)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _seeded_sweep(fam, n, seed, thr, ge, mistake):
    info = {}
    return greedy_sweep(seeded_dets(fam, n, seed), thr, ge, mistake, info), info


def seeded_sweep(fam, n, seed, thr, ge, mistake=None):
    """(sweep, info) of the uncapped statement, computed once per input and reading: 'gt' IS the ge = False sweep, and
    'keep_score_order' only changes how a sweep is reported (cut_sweep)."""
    if mistake == 'gt':
        ge, mistake = False, None
    if mistake == 'keep_score_order':
        mistake = None
    return _seeded_sweep(fam, n, seed, thr, bool(ge), mistake)


def case_dets(fam, n):
    return seeded_dets(fam, n, seed_of(fam, n))


def case_sweep(fam, n, thr, ge, mistake=None):
    """(sweep, info) of the uncapped statement on the case's input: shared by every test that needs it, never modified"""
    return seeded_sweep(fam, n, seed_of(fam, n), thr, ge, mistake)


# which chunk the cap is reached in, per max_keep of a (family, n): 'first' (chunk 0), 'middle', 'last' (the ragged last chunk), 'never'
def cap_place(n, info):
    if not info['cap_reached']:
        return 'never'
    last = (n - 1) // 64
    return 'first' if info['cap_chunk'] == 0 else ('last' if info['cap_chunk'] == last and n % 64 else 'middle')


def first_keep(n, k, survivors):
    """max_keep of a FIRST_CASES entry: 'n' -> n, 's' -> the survivor count (the cap is reached AT the last survivor)"""
    return n if k == 'n' else (survivors if k == 's' else k)


def first_mistakes(fam, n, max_keep, survivors, levels):
    """The mistakes that apply to an hvr_nms_first case (ge): the output order once the boxes returned carry two score levels (equal
    scores are visited in index order, so within one level the two orders coincide: `levels` = distinct scores among the first
    max_keep survivors); the tie rule in the ties family; the IoU mistakes where the cut keeps enough of the sweep for one wrong
    verdict to show -- the cap is not reached (the answer is hvr_nms's) or lies at 1023 and above.  max_keep = 1 in the other
    families returns the best box whatever is planted: such a case is run for its condition (the cap is reached in the first
    chunk) alone."""
    m = []
    if levels >= 2:
        m.append('keep_score_order')
    if fam == 'ties':
        m.append('tie_high_index')
    if max_keep > survivors or max_keep >= 1023:
        m.append('no_plus1')
        if fam != 'degenerate':
            m.append('gt')
    return m


def score_levels(dets, sweep, max_keep):
    idx = sweep[0][:max_keep] if max_keep > 0 else sweep[0]
    return len(set(np.asarray(dets)[idx, 4].tolist()))


def qualifies(fam, n, seed):
    """Does family(fam, n, seed) meet every condition of its hvr_nms cases, is each of them moved by every mistake that applies, and
    the same for its hvr_nms_first cases?  -> (ok, reason)"""
    d = seeded_dets(fam, n, seed)
    if fam == 'float' and not float_margin(d, 0.5) > FLOAT_MARGIN:
        return False, 'a pair within 2^-20 thr of thr'
    for (f, m, thr, ge) in NMS_CASES:
        if (f, m) != (fam, n):
            continue
        sweep, info = seeded_sweep(fam, n, seed, thr, ge)
        for name, holds in nms_conditions(fam, n, thr, ge, info):
            if not holds:
                return False, 'ge=%d: %s' % (ge, name)
        right = cut_sweep(sweep)
        for mis in nms_mistakes(fam, n, thr, ge):
            if cut_sweep(seeded_sweep(fam, n, seed, thr, ge, mis)[0], 0, mis) == right:
                return False, 'ge=%d: %s does not move it' % (ge, mis)
    for (f, m, thr, k) in FIRST_CASES:
        if (f, m) != (fam, n):
            continue
        sweep, info = seeded_sweep(fam, n, seed, thr, True)
        mk = first_keep(n, k, info['survivors'])
        ci = {}
        right = cut_sweep(sweep, mk, None, ci)
        if k == 's' and cap_place(n, ci) != 'last':
            return False, 'max_keep = survivors: the cap is not reached in the last chunk'
        for mis in first_mistakes(fam, n, mk, info['survivors'], score_levels(d, sweep, mk)):
            if cut_sweep(seeded_sweep(fam, n, seed, thr, True, mis)[0], mk, mis) == right:
                return False, 'max_keep=%s: %s does not move it' % (k, mis)
    return True, ''


# ------------------------------------------------------------------------------------------------ cases of hvr_multiclass_nms
MC_SCORE_THR = 0.125        # on the score grid k / 64: scores equal to it exist and must NOT pass (strict >)
MC_LDS_CAP = 160 * 1024 - 3072      # the merge kernel's dynamic LDS (run_multiclass_nms)


def mc_sp2(R, ncls, max_num):
    """run_multiclass_nms' choice: the select list of next_pow2(max_num) entries, or 0 (sort in place) when max_num covers every
    possible survivor or the list does not fit in LDS beside the next_pow2((ncls - 1) * R) candidates (8 bytes an entry each)."""
    np2 = 1
    while np2 < (ncls - 1) * R:
        np2 <<= 1
    sp2 = 1
    while sp2 < max_num:
        sp2 <<= 1
    if max_num >= (ncls - 1) * R or np2 * 8 + sp2 * 8 > MC_LDS_CAP:
        sp2 = 0
    return sp2


def mc_sp2_boundary(R, ncls):
    """the largest max_num that still takes the radix-select cut; max_num + 1 sorts in place"""
    m = 1
    while mc_sp2(R, ncls, m + 1) != 0:
        m += 1
    return m


def mc_case(R, ncls, seed, layout='dense'):
    """-> (boxes [R,4] integer coordinates, scores [R,ncls] on the grid k / 64).  Foreground classes with c % 5 == 2 have no score
    above MC_SCORE_THR (but scores ON it) while their neighbours are full; the other classes carry scores from 1/64 up, so some rows
    fall out by the strict comparison.  layout 'sparse': lattice boxes, most survive (a long list for the max_num cut)."""
    rng = np.random.default_rng([seed, R, ncls, layout == 'sparse'])
    if layout == 'sparse':
        boxes = _lattice(rng, R, max(R, 2))
    else:
        span = 6 + int(np.sqrt(R))
        xy = rng.integers(0, span, (R, 2))
        wh = rng.integers(1, 13, (R, 2))
        boxes = np.concatenate([xy, xy + wh - 1], 1).astype(f32)
    k = rng.integers(1, 65, (R, ncls))
    if layout == 'sparse':
        k = np.maximum(k, 9)                                  # every row a candidate of every class
    empty = [c for c in range(1, ncls) if c % 5 == 2 and ncls > 2]
    k[:, empty] = rng.integers(1, 9, (R, len(empty)))         # <= 8 / 64 = MC_SCORE_THR
    return boxes, (k / 64.0).astype(f32)


MC_SHAPES = [(R, ncls) for R in (1, 63, 64, 65, 300, 511, 512) for ncls in (2, 31)] + [(64, 129), (128, 129)]
MC_IOUS = (0.3, 0.5)
MC_MAX_NUMS = (1, 7, 100)       # + total - 1, total, total + 1 of each case
MC_BOUNDARY_SHAPES = [(300, 31), (128, 129)]        # sparse layout: totals far above the sp2 boundary
# per (R, ncls, layout): the first seed of 1, 2, 3, ... for which mc_qualifies holds (tests/test_nms_refs.py checks exactly that)
MC_SEEDS = {(1, 2, 'dense'): 66, (1, 31, 'dense'): 2, (63, 2, 'dense'): 5, (64, 2, 'dense'): 4, (65, 2, 'dense'): 6, (300, 2, 'dense'): 2,
            (300, 31, 'dense'): 2, (511, 2, 'dense'): 2, (64, 129, 'dense'): 2}


@functools.lru_cache(maxsize=None)
def mc_inputs(R, ncls, layout='dense'):
    b, s = mc_case(R, ncls, MC_SEEDS.get((R, ncls, layout), 1), layout)
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s


@functools.lru_cache(maxsize=None)
def mc_list(R, ncls, iou_thr, layout='dense', mistake=None):
    """(list, info) of the uncut statement on the case's input, computed once"""
    info = {}
    b, s = mc_inputs(R, ncls, layout)
    return multiclass_list(b, s, MC_SCORE_THR, iou_thr, mistake, info), info


def mc_max_nums(total):
    return sorted(set(m for m in MC_MAX_NUMS + (total - 1, total, total + 1) if m > 0))


def mc_conditions(R, ncls, iou_thr, info):
    c = [('scores on score_thr', info['scores_on_thr'] > 0)]
    if ncls >= 31:
        cand = info['candidates']
        c.append(('an empty class between full ones', any(cand[i] == 0 and cand[i - 1] > R // 2 and cand[i + 1] > R // 2
                                                          for i in range(1, len(cand) - 1))))
    if iou_thr == 0.5 and R >= 63:
        c.append(('IoUs exactly on 0.5', info['exact_hits'] > 0))
    if R >= 63:
        c.append(('some suppressed', info['total'] < sum(info['candidates'])))
    return c


def mc_mistakes(R, ncls, iou_thr, max_num, info):
    """The planted mistakes that apply to (case, max_num); info: of multiclass_nms on the case.  Without a cut every reading of the
    class stage shows in the output: the strict score threshold (scores sit on it), the IoU mistakes (0.5 has exact hits), the
    tie rule and the order inside a class.  With a cut the two cut mistakes apply -- 'unstable_cut' where the cut falls between equal
    scores -- and the class-stage ones may hide behind it.  R = 1 has no pair of boxes: only the score threshold applies."""
    if R == 1:
        return ['score_ge_thr'] if not info['cut'] else (['unstable_cut'] if info['cut_tie'] else [])
    if not info['cut']:
        return ['score_ge_thr', 'no_plus1', 'keep_score_order'] + (['tie_high_index'] if mc_ties_expected(R, ncls) else []) + \
            (['gt'] if iou_thr == 0.5 else [])
    return ['cut_before_sort'] + (['unstable_cut'] if info['cut_tie'] else [])


def mc_ties_expected(R, ncls):
    """On the 64-level score grid a tied pair that also overlaps, or a tie exactly at one of six cuts, needs a few hundred candidates to
    be likely: demanded from 300 candidates on."""
    return (ncls - 1) * R >= 300


def same_output(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def _mc_seeded_list(R, ncls, layout, seed, iou_thr, mistake):
    info = {}
    b, s = mc_case(R, ncls, seed, layout)
    return multiclass_list(b, s, MC_SCORE_THR, iou_thr, mistake, info), info, b


def mc_qualifies(R, ncls, layout, seed):
    """-> (ok, reason): every condition of mc_conditions holds at both IoU thresholds, a tie lies at the cut of at least one max_num
    of the case (R >= 63), and every (case, max_num) is moved by each of its mc_mistakes."""
    for iou in MC_IOUS:
        lst, info, b = _mc_seeded_list(R, ncls, layout, seed, iou, None)
        for name, holds in mc_conditions(R, ncls, iou, info):
            if not holds:
                return False, 'iou %g: %s' % (iou, name)
        nums = mc_max_nums(info['total']) if layout == 'dense' else mc_boundary_nums(R, ncls)
        if layout == 'sparse' and info['total'] <= max(nums):
            return False, 'the list is too short for the sp2 boundary'
        tie_seen = False
        for mx in nums:
            ci = dict(info)
            right = cut_list(b, lst, mx, None, ci)
            tie_seen |= ci['cut_tie']
            for mis in mc_mistakes(R, ncls, iou, mx, ci):
                wl = _mc_seeded_list(R, ncls, layout, seed, iou, mis if mis in MISTAKES_NMS + ('score_ge_thr',) else None)[0]
                if same_output(cut_list(b, wl, mx, mis), right):
                    return False, 'iou %g max_num %d: %s does not move it' % (iou, mx, mis)
        if mc_ties_expected(R, ncls) and not tie_seen:
            return False, 'iou %g: no tie at any cut' % iou
    return True, ''


def mc_boundary_nums(R, ncls):
    """one max_num on each side of the switch between the radix-select cut and the in-place sort"""
    m = mc_sp2_boundary(R, ncls)
    return [m, m + 1]
