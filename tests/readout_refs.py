"""Plain float64 statements of the geometry kernels that sit between the MFMA calls of the window path, written from the
definitions and independently of the HIP code, with the per-element error bounds that tests/test_readout_refs.py (CPU) and
tests/test_readout_kernels_gpu.py (GPU) hold the kernels to:

  * RoIAlign forward (roi_align.hip): the interpolation matrix of tests/train_kernel_refs.py and its roi_forward_bound, plus an
    EXACT family (roi_exact_*) on which every intermediate of the kernel is an f32 number, so the result is decided bit for bit;
  * box decode (delta2bbox: det_decode_kernel in misc.hip, rpn_decode_one in nms.hip), class softmax and objectness sigmoid;
  * target encode (bbox2delta: box_targets_kernel) and the "+1" IoU with the max-IoU assignment (targets.hip).

Bounds.  u = 2^-24 is the unit roundoff of f32.  Every quantity is carried as a pair (value, err): the f64 value of the statement
and a bound on |f32 result - value| for ANY f32 evaluation of the same expression tree (class Val):
  * + - * : the operands' errors propagated exactly (|a| eb + |b| ea + ea eb for a product), plus one rounding u (|value| + err);
  * a multiply-add may be fused (one rounding of the sum) or not (the product rounded, then the sum): the unfused bound is the wider
    of the two and is the one carried;
  * scaling by a power of two, negation, min / max / clamp against exact constants: no rounding; min / max / clamp are 1-Lipschitz, so
    the error passes through (the larger of the operands' errors for a two-operand min / max; a clamp maps [v - e, v + e] onto its
    image, so a value cut off with room to spare carries no error);
  * division: correctly rounded, one u;
  * expf / logf: the accuracy contract the device math library is written to, OpenCL C full profile: 3 ulp each (EXP_ULPS,
    LOG_ULPS).  That is the documented contract, not a figure measured on a device.  The same profile lets an implementation
    flush subnormal results to zero, so exp carries an absolute 2^-126 on top;
  * softmax over n classes, score_c = exp(x_c - max) / sum_j exp(x_j - max): the running f32 sum of n terms rounds n - 1 times, each
    term carries (|x_j - max| + 6) u relative (the rounded subtraction moves the exponent by |x - max| u; 3 ulp <= 6 u), the
    numerator the same, the division one more: (n + c) u relative with c = 2 (6 + max_j |x_j - max|) (first order; Val carries
    the second-order terms too).  The bound used is what Val propagates through exactly that tree, which is never larger.
"""
import math

import numpy as np
import torch

from tests import train_kernel_refs as T

U = T.U
EXP_ULPS = 3.0
LOG_ULPS = 3.0
TINY = 2.0 ** -126


def f32c(x):
    """A host constant as the kernels receive it: rounded to f32."""
    return float(np.float32(x))


def ulp32(x):
    """The f32 unit in the last place at magnitude |x| (f64 tensor)."""
    _, e = torch.frexp(x.abs().clamp(min=TINY))
    return torch.ldexp(torch.ones_like(x), e - 24)


class Val(object):
    """value and error bound of one f32 quantity (module docstring)."""

    def __init__(self, v, e=None):
        self.v = v.double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, Val) else Val(x)

    def _rounded(self, v, e_in):
        return Val(v, e_in + U * (v.abs() + e_in))

    def __add__(self, o):
        o = Val.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Val.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Val.of(o)
        return self._rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = Val.of(o)
        assert bool((o.v.abs() > o.e).all()), 'divisor not bounded away from zero'
        v = self.v / o.v
        return self._rounded(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e))

    def scale(self, p):
        """times a power of two: exact."""
        assert math.frexp(p)[0] == 0.5
        return Val(self.v * p, self.e * abs(p))

    def neg(self):
        return Val(-self.v, self.e)

    def clamp(self, min=None, max=None):
        """against exact constants: the image of [v - e, v + e] (1-Lipschitz; no error at all where the whole interval is cut off)."""
        v = self.v.clamp(min=min, max=max)
        up, dn = (self.v + self.e).clamp(min=min, max=max), (self.v - self.e).clamp(min=min, max=max)
        return Val(v, torch.maximum(up - v, v - dn))

    def maximum(self, o):
        return Val(torch.maximum(self.v, o.v), torch.maximum(self.e, o.e))

    def minimum(self, o):
        return Val(torch.minimum(self.v, o.v), torch.maximum(self.e, o.e))

    def exp(self):
        v = self.v.exp()
        e_in = v * torch.expm1(self.e)
        return Val(v, e_in + EXP_ULPS * ulp32(v.abs() + e_in) + TINY)

    def log(self):
        assert bool((self.v > self.e).all())
        v = self.v.log()
        e_in = -torch.log1p(-self.e / self.v)
        return Val(v, e_in + LOG_ULPS * ulp32(v.abs() + e_in))

    def __getitem__(self, i):
        return Val(self.v[i], self.e[i])


def stack(vals, dim=-1):
    return Val(torch.stack([x.v for x in vals], dim), torch.stack([x.e for x in vals], dim))


def ratio(got, val):
    """(worst |got - value| / err, its flat index, how many elements are over) ; an element with err == 0 must be equal."""
    err = (got.double() - val.v).abs()
    r = torch.where(val.e > 0, err / val.e.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float(r.max()), int(r.argmax()), int((r > 1).sum())


# =============================================================================== RoIAlign forward
PH = PW = 7
SCALE = 1 / 16
MAP_B, MAP_H, MAP_W = 3, 13, 17


def roi_family(seed=61):
    """edge_rois + adaptive_rois + roi_cases(60) for the 3 x 13 x 17 maps of the forward tests."""
    return torch.cat([T.edge_rois(MAP_B, MAP_H, MAP_W), T.adaptive_rois(MAP_B, MAP_H, MAP_W), T.roi_cases(MAP_B, MAP_H, MAP_W, 60, seed)])


def nan_rows(A, bins=PH * PW):
    """[rows] True where a bin has no samples (sn_h * sn_w == 0): the mean over nothing, 0 / 0."""
    return ((A.sn_h * A.sn_w) == 0).repeat_interleave(bins)


def live_fraction(A):
    """[rows, 1] f64: live samples / (sn_h * sn_w) per bin (a live sample's four weights add up to one)."""
    ones = torch.ones((A.cols, 1), dtype=torch.float64, device=A.val.device)
    return T.apply(A, ones)


def nhwc_kernel(C, dtype, sample_num, aligned):
    """Which forward kernel the launcher's documented rule selects for an NHWC call (None: refused)."""
    if dtype == torch.float32:
        return 'nhwc<float,4>' if C % 4 == 0 and C // 4 <= 256 else None
    if C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0:
        return 'nhwc_bf16_s2' if sample_num == 2 and aligned else 'nhwc<T,8>'
    if C % 4 == 0 and C // 4 <= 256:
        return 'nhwc<T,4>'
    return None


# ---- the exact family: corners on multiples of 2 px, scale 1/16, 4 x 4 bins, 2 x 2 samples, integer features |f| <= 8
EX_PH = EX_PW = 4
EX_B = 2


def roi_exact_rois(seed=7, n_random=24):
    H, W = MAP_H, MAP_W
    fixed = [
        [0, -20, -20, 43, 43],                      # bin 1: samples on -1, -0.5, 0, ... 2.5
        [1, 220, 156, 283, 219],                    # bin 1: samples on 14 .. 17.5 in x (W - 1, W, past W), 10 .. 13.5 in y
        [0, -18, -18, 13, 13],                      # bin 1/2: samples on -1, -0.75, ..., 0
        [1, 16 * (W - 2) - 2, 16 * (H - 2) - 2, 16 * (W - 2) + 29, 16 * (H - 2) + 29],   # bin 1/2: ... W, W + 0.25 / H, H + 0.25
        [0, 64, 48, 127, 111],                      # interior integers only
        [1, 100, 90, 39, 29],                       # malformed: zero extent, every sample on the start corner
        [0, -60, -60, -29, -29],                    # all samples below -1
        [1, 16 * W + 4, 16 * H + 4, 16 * W + 67, 16 * H + 67],   # all samples past the map
    ]
    g = torch.Generator().manual_seed(seed)
    x1 = 2 * torch.randint(-16, 8 * W + 8, (n_random,), generator=g)
    y1 = 2 * torch.randint(-16, 8 * H + 8, (n_random,), generator=g)
    w = 2 * torch.randint(1, 70, (n_random,), generator=g)
    h = 2 * torch.randint(1, 60, (n_random,), generator=g)
    b = torch.randint(0, EX_B, (n_random,), generator=g)
    rnd = torch.stack([b, x1, y1, x1 + w - 1, y1 + h - 1], 1).float()
    return torch.cat([torch.tensor(fixed, dtype=torch.float32), rnd])


def roi_exact_features(C, seed=9):
    """[B, H, W, C] integers in [-8, 8] as f32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (EX_B, MAP_H, MAP_W, C), generator=g).float()


def _rt(x, what):
    assert torch.equal(x, x.float().double()), 'not an f32 number: ' + what
    return x


def _exact_axis(v, size, mistake):
    """One axis of the bilinear rule from its definition: a coordinate in [-1, size] counts, (-1, 0] reads cell 0, [size - 1, size]
    reads the last cell.  -> (lo, hi, w_lo, w_hi, live)."""
    dead = (v < -1.0) | (v > float(size))
    if mistake == 'border_mut':
        dead = (v < -1.0) | (v > float(size - 1))
    if mistake == 'neg_le':
        dead = (v <= -1.0) | (v > float(size))
    v = v.clamp(min=0.0)
    lo = v.floor()
    top = lo >= size - 1
    lo = torch.where(top, torch.full_like(lo, size - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    frac = torch.where(top, torch.zeros_like(v), v - lo)
    return lo.long(), hi.long(), _rt(1.0 - frac, '1 - l'), _rt(frac, 'l'), ~dead


def roi_exact_matrix(rois, mistake=None):
    """The exact family's interpolation matrix (a train_kernel_refs.RoiMatrix with eps = 0) and its sample coordinates; asserts that
    every intermediate -- corners, extents, bin sizes, sample coordinates by either association, axis weights, tap weights -- equals
    its own f32 round trip."""
    B, H, W, PHh, PWw = EX_B, MAP_H, MAP_W, EX_PH, EX_PW
    r = rois.double()
    K = r.shape[0]
    sc = 1.0 / 16
    coords = {}
    axes = {}
    for name, a, b, size, n_bins in (('x', 1, 3, W, PWw), ('y', 2, 4, H, PHh)):
        start = _rt(r[:, a] * sc, 'start')
        end = _rt(_rt(r[:, b] + 1.0, 'x2 + 1') * sc, 'end')
        ext = _rt((end - start).clamp(min=0.0), 'extent')
        bins = _rt(ext / n_bins, 'bin')
        p = torch.arange(n_bins, dtype=torch.float64)[None, :, None]
        i = torch.arange(2, dtype=torch.float64)[None, None, :]
        pb = _rt(p * bins[:, None, None], 'p * bin')
        base = _rt(start[:, None, None] + pb, 'start + p * bin')
        off = _rt(_rt((i + 0.5) * bins[:, None, None], '(i + .5) * bin') / 2.0, 'offset')
        v = _rt(base + off, 'coordinate')                       # [K, n_bins, 2]
        _rt(start[:, None, None] + _rt(pb + off, 'p * bin + offset'), 'coordinate, other association')
        coords[name] = v
        axes[name] = _exact_axis(v, size, mistake)
    A = T.RoiMatrix(K * PHh * PWw, B * H * W)
    A.sn_h = A.sn_w = torch.full((K,), 2, dtype=torch.long)
    ylo, yhi, ywl, ywh, yok = axes['y']
    xlo, xhi, xwl, xwh, xok = axes['x']
    Y = lambda t: t[:, :, None, :, None]
    X = lambda t: t[:, None, :, None, :]
    shape = (K, PHh, PWw, 2, 2)
    ok = (Y(yok) & X(xok)).double()
    rowi = (torch.arange(K)[:, None, None] * PHh * PWw + torch.arange(PHh)[None, :, None] * PWw + torch.arange(PWw)[None, None, :])[:, :, :, None, None]
    bb = r[:, 0].long()[:, None, None, None, None]
    for yi, wy in ((ylo, ywl), (yhi, ywh)):
        for xi, wx in ((xlo, xwl), (xhi, xwh)):
            w = _rt(Y(wy) * X(wx), 'tap weight') * ok
            assert torch.equal(w * 2.0 ** 14, (w * 2.0 ** 14).round())      # multiples of 2^-14: see roi_exact_statement
            A.row.append(rowi.expand(shape).reshape(-1))
            A.col.append(((bb * H + Y(yi)) * W + X(xi)).expand(shape).reshape(-1))
            A.val.append((w / 4.0).expand(shape).reshape(-1))
            A.eps.append(torch.zeros(shape, dtype=torch.float64).reshape(-1))
    return A.finish(), coords


def roi_exact_statement(A, F):
    """A F for integer features |f| <= 8 ([cols, C]); exact in f32 in ANY order of summation, fused or not: every tap weight is a
    multiple of 2^-14 (asserted in roi_exact_matrix) and at most 1, so every product w f is a multiple of 2^-14, and any partial sum
    of a bin's 16 products is a multiple of 2^-14 of magnitude at most 4 x 8 = 32 < 2^10: 24 bits hold it.  The mean's / 4 is a
    power of two.  Returned in f64; asserted to be an f32 number."""
    Fd = F.double()
    assert torch.equal(Fd, Fd.round()) and float(Fd.abs().max()) <= 8
    return _rt(T.apply(A, F), 'bin mean')


def roi_exact_landmarks(coords):
    """How many sample coordinates of the exact family sit on each landmark of the border rule, per axis."""
    out = {}
    for name, size in (('x', MAP_W), ('y', MAP_H)):
        v = coords[name]
        whole = v == v.floor()
        out[name] = dict(minus_one=int((v == -1).sum()), zero=int((v == 0).sum()),
                         interior=int((whole & (v > 0) & (v < size - 1)).sum()), last=int((v == size - 1).sum()),
                         size=int((v == size).sum()), just_past=int(((v > size) & (v <= size + 0.5)).sum()),
                         inside_last=int(((v > size - 1) & (v < size)).sum()))
    return out


# =============================================================================== box decode
def max_ratio_of(wh_ratio_clip=16 / 1000):
    return f32c(abs(math.log(wh_ratio_clip)))


def _cols(t):
    return [Val(t[..., i]) for i in range(t.shape[-1])]


def delta2bbox(priors, deltas, means, stds, img_shape=None, scale_factor=0.0, wh_ratio_clip=16 / 1000, mistake=None):
    """priors [N, 4] (x1, y1, x2, y2), deltas [N, 4], both f32 -> Val [N, 4].  From the definition: the prior's centre and "+1" size,
    the centre moved by size * d, the size scaled by exp(d) with d clamped to +-max_ratio, corners at centre -+ size / 2 +- 0.5,
    clipped to [0, img - 1] when an image shape (h, w) is given, divided by scale_factor when it is positive."""
    mr = max_ratio_of(wh_ratio_clip)
    x1, y1, x2, y2 = _cols(priors)
    dv = Val.of(deltas)                      # (a Val: deltas that carry an error of their own, for round trips)
    d = [dv[..., i] * f32c(stds[i]) + f32c(means[i]) for i in range(4)]
    one = 0.0 if mistake == 'no_plus1' else 1.0
    out = []
    for lo, hi, dc, ds, lim in ((x1, x2, d[0], d[2], None if img_shape is None else img_shape[1]),
                                (y1, y2, d[1], d[3], None if img_shape is None else img_shape[0])):
        centre = (lo + hi).scale(0.5)
        size = hi - lo + one
        if mistake == 'clamp_after_exp':
            grown = size * ds.exp().clamp(-mr, mr)
        else:
            grown = size * ds.clamp(-mr, mr).exp()
        moved = centre + size * dc
        a = moved - grown.scale(0.5) + 0.5
        b = moved + grown.scale(0.5) - 0.5
        if lim is not None:
            top = float(lim) if mistake == 'clip_to_img' else float(lim) - 1.0
            a, b = a.clamp(0.0, top), b.clamp(0.0, top)
        if scale_factor > 0:
            s = f32c(scale_factor)
            a, b = (a * s, b * s) if mistake == 'mul_scale' else (a / s, b / s)
        out.append((a, b))
    return stack([out[0][0], out[1][0], out[0][1], out[1][1]])


def softmax(logits):
    """logits [R, n] f32 -> Val [R, n] (module docstring: the running sum in class order)."""
    x = [Val(logits[:, c]) - Val(logits.double().max(1).values) for c in range(logits.shape[1])]
    e = [t.exp() for t in x]
    s = e[0]
    for t in e[1:]:
        s = s + t
    return stack([t / s for t in e])


def sigmoid(logit):
    return Val(1.0) / (Val(logit).neg().exp() + 1.0)


def clamp_census(deltas, means, stds, wh_ratio_clip=16 / 1000):
    """(below, inside, above): how many dw / dh land below -max_ratio, inside, above +max_ratio."""
    mr = max_ratio_of(wh_ratio_clip)
    d = torch.stack([deltas[:, i].double() * f32c(stds[i]) + f32c(means[i]) for i in (2, 3)], 1)
    return int((d < -mr).sum()), int(((d > -mr) & (d < mr)).sum()), int((d > mr).sum())


def det_case(R, seed, ldl=160, cls_off=3, reg_off=40, ncls=31, img=(208, 272)):
    """(wide [R, ldl] f32, rois [R, 5]): class logits in columns cls_off.., deltas in reg_off..; row maxima of the logits at +80
    and -80 in turn; deltas so that std-scaled dw / dh land on both sides of max_ratio; RoIs inside the image and across its border."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn((R, ldl), generator=g) * 50.0
    cls = torch.randn((R, ncls), generator=g) * 3.0
    cls = cls - cls.max(1, keepdim=True).values + torch.where(torch.arange(R) % 2 == 0, 80.0, -80.0)[:, None]
    wide[:, cls_off:cls_off + ncls] = cls
    d = torch.randn((R, 4), generator=g)
    d[:, 2:] = (torch.rand((R, 2), generator=g) * 2 - 1) * 30.0          # x std 0.2: +-6 around the clamp at 4.135
    wide[:, reg_off:reg_off + 4] = d
    xy = torch.rand((R, 2), generator=g) * torch.tensor([img[1] + 60.0, img[0] + 60.0]) - 40.0
    wh = torch.rand((R, 2), generator=g) * 90.0 + 1.0
    rois = torch.cat([torch.zeros(R, 1), xy, xy + wh], 1)
    return wide.float(), rois.float()


DET_MEANS, DET_STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)


# =============================================================================== "+1" IoU and the max-IoU assignment
def iou(a, b, mistake=None):
    """a Val [n, 4], b Val [k, 4] -> Val [n, k]: intersection over union of pixel boxes (extent x2 - x1 + 1)."""
    one = 0.0 if mistake == 'no_plus1' else 1.0
    A = [a[:, i][:, None] for i in range(4)]
    B = [b[:, i][None, :] for i in range(4)]
    w = (A[2].minimum(B[2]) - A[0].maximum(B[0]) + one).clamp(min=0.0)
    h = (A[3].minimum(B[3]) - A[1].maximum(B[1]) + one).clamp(min=0.0)
    inter = w * h
    area_a = (A[2] - A[0] + one) * (A[3] - A[1] + one)
    area_b = (B[2] - B[0] + one) * (B[3] - B[1] + one)
    return inter / (area_a + area_b - inter)


def max_iou_assign(boxes, gts, pos_thr, neg_thr, min_pos, valid=None):
    """The max-IoU assigner in f64 -> (gt_inds int64 [n], max_overlaps Val [n], margin).  -1: ignored (also rows masked by `valid`),
    0: background (max IoU in [neg_lo, neg_hi)), g + 1: max IoU >= pos_thr (first maximal gt), and every box whose IoU with gt g
    equals that gt's maximum over the valid boxes, where that maximum is >= min_pos (later gts override).
    margin: the smallest distance, minus the IoU bound(s), of any comparison the result depends on -- max IoU against pos_thr, both
    ends of the background interval (an end <= 0 decides nothing: an IoU is never negative), a gt's maximum against min_pos, a box's
    best gt against its runner-up (where the box is positive), a gt's maximum against the best box that is no bit-for-bit copy of the
    maximal one.  Positive: any f32 evaluation within the bound assigns identically."""
    n, k = boxes.shape[0], gts.shape[0]
    ov = iou(Val(boxes), Val(gts))
    ok = torch.ones(n, dtype=torch.bool) if valid is None else valid.bool()
    lo, hi = (0.0, float(neg_thr)) if isinstance(neg_thr, (int, float)) else (float(neg_thr[0]), float(neg_thr[1]))
    pos_thr, lo, hi, min_pos = f32c(pos_thr), f32c(lo), f32c(hi), f32c(min_pos)
    mv, arg = ov.v.max(1)
    me = ov.e.gather(1, arg[:, None])[:, 0]
    inds = torch.full((n,), -1, dtype=torch.long)
    inds[ok & (mv >= lo) & (mv < hi)] = 0
    pos = ok & (mv >= pos_thr)
    inds[pos] = arg[pos] + 1
    margin = float('inf')
    emax = float(ov.e.max())
    for thr in (pos_thr, lo, hi):
        if thr > 0 and bool(ok.any()):
            margin = min(margin, float(((mv - thr).abs() - me)[ok].min()))
    if k > 1 and bool(pos.any()):
        top2 = ov.v.topk(2, dim=1).values
        margin = min(margin, float((top2[:, 0] - top2[:, 1])[pos].min()) - 2 * emax)
    ovv = torch.where(ok[:, None], ov.v, torch.zeros_like(ov.v))
    for g in range(k):
        col = ovv[:, g]
        m, at = col.max(0)
        margin = min(margin, abs(float(m) - min_pos) - emax)
        if float(m) >= min_pos:
            same = ok & (col == m)
            inds[same] = g + 1
            copies = (boxes[:, :4] == boxes[at, :4]).all(1)
            others = col[ok & ~copies]
            if others.numel():
                margin = min(margin, float(m - others.max()) - 2 * emax)
    return inds, Val(torch.where(ok, mv, torch.full_like(mv, -1.0)), torch.where(ok, me, torch.zeros_like(me))), margin


def assign_case(n, k, seed, img=(600, 1000)):
    """boxes [n, 5] (an RoI tensor: the boxes are columns 1..4), gts [k, 4], valid [n]: jittered copies of the gts (high IoU), random
    boxes, and for gt 0 a box duplicated bit for bit (rows 0 and n - 1 when n > 2)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((k, 2), generator=g) * torch.tensor([img[1] - 200.0, img[0] - 200.0]) + 20.0
    wh = torch.rand((k, 2), generator=g) * 150.0 + 30.0
    gts = torch.cat([c, c + wh], 1).round()
    src = torch.randint(0, k, (n,), generator=g)
    jit = torch.randn((n, 4), generator=g) * (torch.rand((n, 1), generator=g) * 25.0)
    b = gts[src] + jit
    rnd = torch.rand((n,), generator=g) < 0.3
    rc = torch.rand((n, 2), generator=g) * torch.tensor([img[1] - 100.0, img[0] - 100.0])
    b[rnd] = torch.cat([rc, rc + torch.rand((n, 2), generator=g) * 200.0 + 5.0], 1)[rnd]
    b = torch.cat([torch.minimum(b[:, :2], b[:, 2:] - 2.0), b[:, 2:]], 1)
    if n > 2:
        b[0] = gts[0] + torch.tensor([3.0, -2.0, 1.5, 2.5])
        b[n - 1] = b[0]
    rois = torch.cat([torch.randint(0, 3, (n, 1), generator=g).float(), b], 1).float()
    valid = torch.rand((n,), generator=g) < 0.85
    if n > 2:
        valid[0] = valid[n - 1] = True
    return rois, gts.float(), valid


# =============================================================================== target encode
def bbox2delta(p, g, means, stds, mistake=None):
    """proposals p [N, 4], ground truths g [N, 4] f32 -> Val [N, 4]: ((gx - px) / pw, (gy - py) / ph, log(gw / pw), log(gh / ph)) with
    "+1" sizes, then (d - mean) / std."""
    P, G = _cols(p), _cols(g)
    out = [None] * 4
    for i, (lo, hi) in enumerate(((0, 2), (1, 3))):
        pc, gc = (P[lo] + P[hi]).scale(0.5), (G[lo] + G[hi]).scale(0.5)
        ps, gs = P[hi] - P[lo] + 1.0, G[hi] - G[lo] + 1.0
        out[i] = (gc - pc) / ps
        out[i + 2] = (ps / gs).log() if mistake == 'inverted_log' else (gs / ps).log()
    if mistake == 'no_stds':
        return stack([out[i] - f32c(means[i]) for i in range(4)])
    return stack([(out[i] - f32c(means[i])) / f32c(stds[i]) for i in range(4)])


def box_targets(boxes, gts, gt_labels, gt_inds, inds, counts, means, stds, pos_weight, scatter):
    """The sampled boxes' targets: rows j < counts[0] of `inds` are positives (label of their gt, or 1; weight pos_weight if positive
    else 1; the encoded deltas with weight 1), the next counts[1] are negatives (label 0, label weight 1), everything else zero.
    scatter: row inds[j] of n rows, else row j of len(inds) rows.  -> (labels, label_w, Val bbox_t, bbox_w)."""
    n, num = boxes.shape[0], inds.numel()
    rows = n if scatter else num
    np_, nn = int(counts[0]), int(counts[1])
    labels = torch.zeros(rows, dtype=torch.long)
    lw = torch.zeros(rows, dtype=torch.float64)
    bt, be = torch.zeros((rows, 4), dtype=torch.float64), torch.zeros((rows, 4), dtype=torch.float64)
    bw = torch.zeros((rows, 4), dtype=torch.float64)
    pi, ni = inds[:np_], inds[np_:np_ + nn]
    pr = pi if scatter else torch.arange(np_)
    nr = ni if scatter else torch.arange(np_, np_ + nn)
    lw[nr] = 1.0
    if np_:
        gi = gt_inds[pi] - 1
        d = bbox2delta(boxes[pi], gts[gi], means, stds)
        bt[pr], be[pr], bw[pr] = d.v, d.e, 1.0
        labels[pr] = gt_labels[gi] if gt_labels is not None else 1
        lw[pr] = 1.0 if pos_weight <= 0 else float(pos_weight)
    return labels, lw, Val(bt, be), bw


def targets_case(n, k, seed):
    """(boxes [n, 4], gts [k, 4], gt_labels [k], gt_inds [n] in 1..k, inds: a permutation of n): positive-size boxes near their gt."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((k, 2), generator=g) * torch.tensor([800.0, 400.0])
    gts = torch.cat([c, c + torch.rand((k, 2), generator=g) * 180.0 + 8.0], 1).float()
    gt_inds = torch.randint(1, k + 1, (n,), generator=g)
    s = (gts[gt_inds - 1][:, 2:] - gts[gt_inds - 1][:, :2])
    b0 = gts[gt_inds - 1][:, :2] + torch.randn((n, 2), generator=g) * 0.2 * s
    b1 = b0 + s * torch.exp(torch.randn((n, 2), generator=g) * 0.4)
    boxes = torch.cat([b0, b1], 1).float()
    return boxes, gts, torch.randint(1, 31, (k,), generator=g), gt_inds, torch.randperm(n, generator=g)


# =============================================================================== RPN proposals
RPN_H, RPN_W, RPN_STRIDE = 10, 12, 16
RPN_IMG = (RPN_H * RPN_STRIDE, RPN_W * RPN_STRIDE)
RPN_NMS_THR = 0.3


def rpn_base_anchors(A):
    """[A, 4] integer base anchors (three shapes, repeated at growing sizes)."""
    out = []
    for a in range(A):
        half_w, half_h = ((12, 6), (8, 8), (6, 12))[a % 3]
        m = 1 + a // 3
        out.append([-half_w * m + 8, -half_h * m + 8, half_w * m + 7, half_h * m + 7])
    return torch.tensor(out, dtype=torch.float32)


def rpn_anchors(base, H=RPN_H, W=RPN_W, stride=RPN_STRIDE):
    """[H * W * A, 4] in (y, x, anchor) order: the base anchors shifted to every cell (integers: exact in f32)."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    shift = torch.stack([xs, ys, xs, ys], -1).reshape(-1, 1, 4).float() * stride
    out = (shift + base[None]).reshape(-1, 4)
    assert torch.equal(out, out.round())
    return out


def rpn_frame(A, seed, exact=False):
    """(cls [H*W*A] logits, reg [H*W*A, 4]) of one frame: a permutation of an even grid on [-4, 4] (sigmoids far more than an ulp apart:
    asserted by rpn_statement), moderate deltas with one of dw / dh beyond the clamp for a few anchors.  exact: dw = dh = 0 and dyadic
    dx, dy."""
    g = torch.Generator().manual_seed(seed)
    n = RPN_H * RPN_W * A
    cls = torch.linspace(-4.0, 4.0, n)[torch.randperm(n, generator=g)]
    if exact:
        reg = torch.zeros((n, 4))
        reg[:, :2] = torch.randint(-1, 3, (n, 2), generator=g).float() / 16.0      # (too small to land two anchors on one box)
    else:
        reg = torch.randn((n, 4), generator=g) * 0.3
        far = torch.rand((n,), generator=g) < 0.03
        axis = torch.randint(2, 4, (n,), generator=g)
        val = (4.3 + torch.rand((n,), generator=g) * 2.0) * torch.where(torch.rand((n,), generator=g) < 0.5, -1.0, 1.0)
        reg.scatter_(1, axis[:, None], torch.where(far, val, reg.gather(1, axis[:, None])[:, 0])[:, None])
    return cls.float(), reg.float()


def rpn_case(T_, A, seeds, exact=False):
    """T frames stacked: (cls [T, H*W*A], reg [T, H*W*A, 4]) from the first T of `seeds` (RPN_SEEDS: frame seeds for which the
    conditions of rpn_statement on the inputs hold; test_readout_refs.py checks every one of them)."""
    frames = [rpn_frame(A, s, exact) for s in seeds[:T_]]
    assert len(frames) == T_
    return torch.stack([f[0] for f in frames]), torch.stack([f[1] for f in frames])


def rpn_statement(cls, reg, base, nms_pre, nms_post, max_num, nms_thr=RPN_NMS_THR, img=RPN_IMG):
    """One frame (cls [n], reg [n, 4]) in f64: sigmoid, the nms_pre best (all, in anchor order, when there are no more than nms_pre),
    delta2bbox (means 0, stds 1, clipped to the image), greedy NMS in score order (IoU >= thr suppresses), the first nms_post
    survivors, the max_num best of them in score order.
    -> dict(order: anchor index per output row, boxes Val [m, 4], scores Val [m], score_gap, nms_margin, distinct).
    score_gap: the smallest gap between neighbouring sigmoids minus both their bounds (asserted >= 64 u: the selection and the order are
    decided); nms_margin: min over the pairs of decoded boxes of |IoU - thr| - (IoU bound from the box bounds); distinct: no two decoded
    boxes identical."""
    n = cls.numel()
    sc = sigmoid(cls)
    srt = torch.argsort(sc.v, descending=True, stable=True)
    gaps = sc.v[srt][:-1] - sc.v[srt][1:] - sc.e[srt][:-1] - sc.e[srt][1:]
    score_gap = float(gaps.min())
    assert score_gap >= 64 * U, score_gap
    sel = srt[:nms_pre] if n > nms_pre else torch.arange(n)
    anchors = rpn_anchors(base)
    boxes = delta2bbox(anchors[sel], reg[sel], (0, 0, 0, 0), (1, 1, 1, 1), img)
    ov = iou(boxes, boxes)
    m = sel.numel()
    off = ~torch.eye(m, dtype=torch.bool)
    nms_margin = float(((ov.v - f32c(nms_thr)).abs() - ov.e)[off].min())
    distinct = bool(((boxes.v[:, None, :] != boxes.v[None, :, :]).any(-1) | ~off).all())
    by_score = torch.argsort(sc.v[sel], descending=True, stable=True)
    hit = ov.v >= f32c(nms_thr)
    alive = torch.ones(m, dtype=torch.bool)
    keep = []
    for i in by_score.tolist():
        if alive[i]:
            keep.append(i)
            alive &= ~hit[i]
    keep = torch.tensor(keep[:nms_post][:max_num], dtype=torch.long)
    return dict(order=sel[keep], boxes=boxes[keep], scores=sc[sel[keep]], score_gap=score_gap, nms_margin=nms_margin, distinct=distinct)


def rpn_regime(n_anchor, nms_pre, T_, nms_post, wide_frames):
    """hvr_rpn_proposals' rule: 'unsorted' (no selection), 'wide' (chip-wide kernels) or 'workgroup' (one workgroup per frame)."""
    if n_anchor <= nms_pre:
        return 'unsorted'
    return 'wide' if T_ <= wide_frames and 0 < nms_post <= 1024 else 'workgroup'


RPN_NMS_POST, RPN_MAX_NUM = 1000, 300
# frame seeds, per (A, nms_pre, exact), for which the conditions of rpn_statement on the inputs hold (found by trying 1, 2, 3, ... in turn)
RPN_SEEDS = {(3, 64, False): [1, 2, 3, 4, 5], (3, 64, True): [1, 2, 3, 4, 5], (3, 6000, False): [1, 2, 3, 4, 5], (3, 6000, True): [1, 2, 3, 4, 5],
             (12, 64, False): [1, 2, 3, 4, 5], (12, 64, True): [2, 3, 5, 9, 10], (12, 6000, False): [1, 2, 7, 8, 10]}
# (A, T, nms_pre, exact): the calls of the GPU test; the exact ones reach all three regimes (chip-wide, one workgroup, no selection)
RPN_CASES = [(A, T_, nms_pre, False) for A in (3, 12) for T_ in (1, 5) for nms_pre in (64, 6000)] + \
            [(3, 1, 64, True), (12, 5, 64, True), (3, 5, 6000, True)]

# (n, k, seed, pos_iou_thr, neg_iou_thr, min_pos_iou)
ASSIGN_CASES = [(n, k, 7 * n + k, 0.7, 0.3, 0.3) if k == 1 else (n, k, 7 * n + k, 0.5, (0.1, 0.5), 0.5)
                for n in (1, 255, 256, 257, 1000) for k in (1, 256)]
