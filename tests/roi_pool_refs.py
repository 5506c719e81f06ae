"""The statement of RoI max pooling (include/hvr_hip.h, hvr_roi_pool_fwd / hvr_roi_pool_bwd) in numpy, its planted mistakes, and the
cases the CPU and GPU tests share.

The reference's kernel is CUDA and produces no outputs where these tests run, so -- as for RoIAlign -- the statement is the
reference: the geometry in np.float32, operation by operation as the header writes it, the maximum and the argmax by explicit loops
over a bin's pixels (h outer, w inner, strict `>`: the first pixel that attains the maximum).  Parity to the reference's binary is not
pinned by these tests.
"""
import functools

import numpy as np

f32 = np.float32

B, H, W, SCALE = 2, 9, 11, 1.0 / 16          # the repository's small pooling shape (tests/dpool_refs.py)
OUT_SIZES = ((7, 7), (2, 3))
LEVELS = np.array([-4.0, -3.5, -3.0, -2.5, -2.0, -1.5, -1.0, -0.5])   # exact in bf16, f16 and f32; all below zero; ties are frequent
CASES = {   # name -> (C, K, constant frame); 96 channels = 12 lanes per pixel (24 in f32), no divisor of 256
    'c8': (8, 40, False), 'c64': (64, 40, True), 'c96': (96, 40, False), 'c256': (256, 40, False), 'wide': (512, 3, False),
}
WIDE_PICK = ('whole', 'straddle_left', 'fma_x0')

# x1, x2 at scale 1/16, PW = 7: the last bin differs between the stated (every operation rounded) and the contracted evaluation
FMA_SENSITIVE = ((-39.0, 31.0), (-39.0, 95.0), (-37.0, 15.0))

FWD_MISTAKES = ('round_first', 'no_plus1', 'ge', 'zero_init', 'floor_end', 'clamp_w1', 'batch_offset', 'fma', 'malformed_1x1')
BWD_MISTAKES = ('minus1_to_0',)


def _edges(n_bins, size, r1, r2, mistake=None, contracted=False):
    """One axis: [(start, end)] of the n_bins bins of a RoI side [r1, r2) (f32, map units) on an axis of `size` cells."""
    rw = f32(r2 - r1)
    if mistake == 'malformed_1x1' and not rw > 0:
        rw = f32(1.0)
    bw = f32(rw / f32(n_bins))
    hi = f32(size - 1 if mistake == 'clamp_w1' else size)
    out = []
    for p in range(n_bins):
        if contracted or mistake == 'fma':   # one rounding: the exact product plus r1, then f32
            a = f32(np.float64(f32(p)) * np.float64(bw) + np.float64(r1))
            b = f32(np.float64(f32(p + 1)) * np.float64(bw) + np.float64(r1))
        else:
            a = f32(f32(f32(p) * bw) + r1)
            b = f32(f32(f32(p + 1) * bw) + r1)
        s = np.floor(a)
        e = np.floor(b) if mistake == 'floor_end' else np.ceil(b)
        s = min(max(s, f32(0)), hi)
        e = min(max(e, f32(0)), hi)
        out.append((int(s), int(e)))
    return out


def roi_geometry(roi, n_frames, height, width, PH, PW, scale, mistake=None, contracted=False):
    """-> (frame or None, malformed, x edges [PW], y edges [PH]) of one RoI (b, x1, y1, x2, y2)."""
    s = f32(scale)
    bf, x1, y1, x2, y2 = [f32(v) for v in roi]
    if mistake == 'round_first':
        x1, y1, x2, y2 = [f32(np.round(v)) for v in (x1, y1, x2, y2)]
    one = f32(0.0 if mistake == 'no_plus1' else 1.0)
    rx1, ry1 = f32(x1 * s), f32(y1 * s)
    rx2, ry2 = f32(f32(x2 + one) * s), f32(f32(y2 + one) * s)
    frame = int(bf) if (bf >= 0 and bf < n_frames) else None
    malformed = not (f32(rx2 - rx1) > 0 and f32(ry2 - ry1) > 0)
    if mistake == 'malformed_1x1':
        malformed = False
    return (frame, malformed or frame is None, _edges(PW, width, rx1, rx2, mistake, contracted),
            _edges(PH, height, ry1, ry2, mistake, contracted))


def pool_statement(feat, rois, PH, PW, scale, mistake=None):
    """feat [B,H,W,C] (numpy, any float dtype; values are compared as they are), rois [K,5] -> (values [K,PH,PW,C] of feat's dtype,
    argmax [K,PH,PW,C] int32, record) with record = dict(empty [K,PH,PW] bool, area [K,PH,PW] int, ties [K,PH,PW,C] int = pixels of
    the bin that attain the maximum, malformed [K] bool = malformed or a batch index outside [0, B))."""
    nb, h, w, C = feat.shape
    K = rois.shape[0]
    val = np.zeros((K, PH, PW, C), dtype=feat.dtype)
    arg = np.full((K, PH, PW, C), -1, dtype=np.int32)
    rec = dict(empty=np.ones((K, PH, PW), dtype=bool), area=np.zeros((K, PH, PW), dtype=np.int64),
               ties=np.zeros((K, PH, PW, C), dtype=np.int64), malformed=np.zeros(K, dtype=bool))
    for k in range(K):
        frame, bad, xe, ye = roi_geometry(rois[k], nb, h, w, PH, PW, scale, mistake)
        rec['malformed'][k] = bad
        if bad:
            continue
        for ph in range(PH):
            ys, ye_ = ye[ph]
            for pw in range(PW):
                xs, xe_ = xe[pw]
                if xe_ <= xs or ye_ <= ys:
                    continue
                rec['empty'][k, ph, pw] = False
                rec['area'][k, ph, pw] = (ye_ - ys) * (xe_ - xs)
                if mistake == 'zero_init':
                    m, idx = np.zeros(C, dtype=feat.dtype), np.full(C, -1, dtype=np.int32)
                else:
                    m, idx = feat[frame, ys, xs].copy(), np.full(C, ys * w + xs, dtype=np.int32)
                for hh in range(ys, ye_):
                    for ww in range(xs, xe_):
                        v = feat[frame, hh, ww]
                        gt = (v >= m) if mistake == 'ge' else (v > m)
                        m = np.where(gt, v, m)
                        idx = np.where(gt, np.int32(hh * w + ww), idx)
                rec['ties'][k, ph, pw] = (feat[frame, ys:ye_, xs:xe_].reshape(-1, C) == m).sum(0)
                if mistake == 'batch_offset':
                    idx = np.where(idx >= 0, idx + np.int32(frame * h * w), idx)
                val[k, ph, pw], arg[k, ph, pw] = m, idx
    return val, arg, rec


def backward_statement(grad_out, rois, argmax, n_frames, height, width, mistake=None):
    """The f64 scatter grad_feat[b][argmax][c] += grad_out[k][ph][pw][c] over argmax >= 0 (a batch index outside [0, B) never carries
    one) -> (grad [B,H,W,C] f64, n [B,H,W,C] = terms per element, sabs [B,H,W,C] = sum |g| per element)."""
    K, PH, PW, C = grad_out.shape
    g = np.zeros((n_frames, height * width, C), dtype=np.float64)
    n = np.zeros(g.shape, dtype=np.int64)
    sabs = np.zeros(g.shape, dtype=np.float64)
    go = np.asarray(grad_out, dtype=np.float64)
    a = np.asarray(argmax, dtype=np.int64)
    if mistake == 'minus1_to_0':
        a = np.where(a < 0, 0, a)
    c = np.arange(C)
    for k in range(K):
        bf = f32(rois[k][0])
        if not (bf >= 0 and bf < n_frames):
            assert (np.asarray(argmax[k]) < 0).all()
            if mistake != 'minus1_to_0':
                continue
            bf = 0
        b = int(bf)
        for ph in range(PH):
            for pw in range(PW):
                ok = a[k, ph, pw] >= 0
                np.add.at(g[b], (a[k, ph, pw][ok], c[ok]), go[k, ph, pw][ok])
                np.add.at(n[b], (a[k, ph, pw][ok], c[ok]), 1)
                np.add.at(sabs[b], (a[k, ph, pw][ok], c[ok]), np.abs(go[k, ph, pw][ok]))
    shape = (n_frames, height, width, C)
    return g.reshape(shape), n.reshape(shape), sabs.reshape(shape)


# ------------------------------------------------------------------------------------------------ cases
def prescribed_rois():
    """[(family, (b, x1, y1, x2, y2))]: the families every case carries, on the 9 x 11 map at scale 1/16 (144 x 176 image pixels)."""
    r = [('whole', (0, 0, 0, 175, 143)),
         ('off_left', (1, -100, 20, -40, 90)), ('off_right', (0, 200, 20, 260, 90)),
         ('off_top', (1, 20, -90, 120, -30)), ('off_bottom', (0, 20, 170, 120, 230)),
         ('straddle_left', (1, -50, 30, 60, 100)), ('straddle_right', (0, 120, 30, 230, 100)),
         ('straddle_top', (1, 30, -50, 100, 60)), ('straddle_bottom', (0, 30, 100, 100, 200)),
         ('narrow', (1, 50.0, 40.0, 50.2, 90.0)),
         ('malformed_x', (0, 60, 20, 40, 90)), ('malformed_y', (1, 20, 90, 100, 60)), ('malformed_zero', (0, 41, 20, 40, 90)),
         ('batch_minus', (-1, 10, 10, 100, 100)), ('batch_past', (B, 10, 10, 100, 100))]
    for i, (a, b) in enumerate(FMA_SENSITIVE):
        r.append(('fma_x%d' % i, (i % 2, a, 16, b, 111)))
        r.append(('fma_y%d' % i, (1 - i % 2, 16, a, 143, b)))
    r += [('aligned0', (0, 16, 32, 47, 111)), ('aligned1', (1, 0, 0, 111, 111)), ('aligned2', (0, 64, 16, 175, 127)), ('aligned3', (1, 32, 48, 143, 63))]
    return r


def make_case(name):
    return _make_case(name)


@functools.lru_cache(maxsize=None)
def _make_case(name):
    """dict(feat [B,H,W,C] f64 (values exact in every dtype), rois [K,5] f32, family {name: row}, C, K); the family conditions are
    asserted on the statement's own record."""
    C, K, constant = CASES[name]
    rng = np.random.RandomState(1000 + C)
    feat = LEVELS[rng.randint(0, len(LEVELS), size=(B, H, W, C))]
    if constant:
        feat[1] = -2.0
    pres = prescribed_rois()
    if name == 'wide':
        pres = [p for p in pres if p[0] in WIDE_PICK]
    rows = [p[1] for p in pres]
    while len(rows) < K:   # seeded random boxes, a few px to most of the image, up to 30 px off it
        x1, y1 = rng.uniform(-30, 170), rng.uniform(-30, 140)
        rows.append((rng.randint(0, B), x1, y1, x1 + rng.uniform(1, 120), y1 + rng.uniform(1, 100)))
    assert len(rows) == K
    case = dict(name=name, feat=feat, rois=np.array(rows, dtype=np.float32), family={p[0]: i for i, p in enumerate(pres)}, C=C, K=K)
    check_families(case)
    return case


@functools.lru_cache(maxsize=None)
def statement(name, PH, PW, mistake=None):
    c = make_case(name)
    return pool_statement(c['feat'], c['rois'], PH, PW, SCALE, mistake)


def check_families(case):
    """The prescribed families are present by construction; this asserts it on the statement's record (at 7 x 7 bins)."""
    fam, rois = case['family'], case['rois']
    val, arg, rec = pool_statement(case['feat'][..., :8], rois, 7, 7, SCALE)
    empty, area = rec['empty'], rec['area']
    for name, k in fam.items():
        if name == 'whole':
            assert not empty[k].any() and not rec['malformed'][k]
            _, _, xe, ye = roi_geometry(rois[k], B, H, W, 7, 7, SCALE)
            assert xe[0][0] == 0 and xe[-1][1] == W and ye[0][0] == 0 and ye[-1][1] == H
        elif name.startswith('off_'):
            assert empty[k].all() and not rec['malformed'][k], name
        elif name.startswith('straddle_'):
            assert empty[k].any() and not empty[k].all(), name
        elif name == 'narrow':
            assert f32(f32(f32(rois[k][3] + f32(1)) * f32(SCALE)) - f32(rois[k][1] * f32(SCALE))) < f32(0.1) and not empty[k].all()
        elif name.startswith('malformed') or name.startswith('batch_'):
            assert rec['malformed'][k] and empty[k].all() and (arg[k] == -1).all() and not val[k].any(), name
            if name == 'malformed_zero':
                assert rois[k][3] + 1 == rois[k][1]
        elif name.startswith('fma_'):
            stated = roi_geometry(rois[k], B, H, W, 7, 7, SCALE)
            fused = roi_geometry(rois[k], B, H, W, 7, 7, SCALE, contracted=True)
            axis = 2 if name[4] == 'x' else 3
            assert stated[axis] != fused[axis] and stated[5 - axis] == fused[5 - axis], (name, stated, fused)
        elif name.startswith('aligned'):
            x1, y1, x2, y2 = rois[k][1:]
            assert all(float(v) % 16 == 0 for v in (x1, y1, x2 + 1, y2 + 1)) and not empty[k].all()
    assert area.max() > 1 and (area == 1).any()


def grad_out_ints(shape, seed):
    """Small integers: every partial sum of a map element stays far below 2^24, so f32 accumulation is exact in any order."""
    return np.random.RandomState(seed).randint(-8, 9, size=shape).astype(np.float64)


def grad_out_normal(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32).astype(np.float64)
