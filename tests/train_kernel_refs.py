"""Plain float64 statements of the training-step kernels, written independently of the HIP code, and the error bounds the
tests in test_train_kernel_refs.py (CPU) and test_train_kernels_gpu.py (GPU) hold the kernels to.

RoIAlign (roi_align.hip, legacy "+1 pixel" convention) is stated as a sparse interpolation matrix A: row (roi, ph, pw),
column (b, y, x), entry = bilinear weight / sample count, summed over the bin's samples.  Forward = A F, backward = A^T G.
The sample coordinates are the f32 statement of roi_align_kernel.cu (the geometry IS f32 arithmetic there); everything after
them -- tap weights, products, sums -- is exact or f64.  A compiler may fuse `start + ph * bin` into one multiply-add; where
the fused and the unfused f32 coordinate differ (by eps), a tap weight moves by at most eps_y + eps_x (each axis weight is
1-Lipschitz in its coordinate and at most 1), and that allowance is carried per tap in `eps`.
"""
import math

import torch

U = 2.0 ** -24          # unit roundoff of f32 (round to nearest)
C_ROI = 2.0             # the constant c of the RoIAlign bounds: (n + 4) u covers the atomic sum (n - 1 roundings) and up to
                        # five roundings inside one contribution (axis weights, their sum when merged, two products, / count)


def _f32(t):
    return t.to(torch.float32)


class RoiMatrix(object):
    """A in COO form (duplicates kept: one entry per (sample, tap), which is what the kernels add one by one).
    row / col: int64 [nnz]; val, eps: f64 [nnz]; rows = K * PH * PW, cols = B * H * W; sn_h / sn_w: [K] samples per bin;
    stats: how many samples fall under each border rule, and merging_bins (see merge_path_stats)."""

    def __init__(self, rows, cols):
        self.rows, self.cols = rows, cols
        self.row, self.col, self.val, self.eps = [], [], [], []
        self.merging_bins = 0
        self.stats = dict(y_neg=0, x_neg=0, y_clamped=0, x_clamped=0, y_dead_only=0, x_dead_only=0, dead=0, live=0)

    def finish(self):
        cat = lambda xs, dt: torch.cat(xs) if xs else torch.zeros(0, dtype=dt)
        self.row, self.col = cat(self.row, torch.int64), cat(self.col, torch.int64)
        self.val, self.eps = cat(self.val, torch.float64), cat(self.eps, torch.float64)
        return self

    def to(self, device):
        for k in ('row', 'col', 'val', 'eps'):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def n_cell(self):
        """Contributions per column (what the backward's atomics add into one cell, before any merging)."""
        return torch.bincount(self.col, minlength=self.cols)

    def n_row(self):
        return torch.bincount(self.row, minlength=self.rows)

    def sparse(self):
        return torch.sparse_coo_tensor(torch.stack([self.row, self.col]), self.val, (self.rows, self.cols)).coalesce()


def _axis(v, size, border_mut=False):
    """One axis of make_tap on f32 coordinates v (any shape): (lo, hi, w_lo, w_hi, ok); weights f64 and exact."""
    ok = ~((v < -1.0) | (v > float(size - 1 if border_mut else size)))
    v = torch.where(v <= 0, torch.zeros_like(v), v).double()
    lo = v.floor().long()
    top = lo >= size - 1
    lo = torch.where(top, torch.full_like(lo, size - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    v = torch.where(top, lo.double(), v)
    l = v - lo.double()
    return lo, hi, 1.0 - l, l, ok


def _coords(start, bins, n_bins, sn, off_frac=0.5):
    """f32 sample coordinates [k, n_bins, sn] as roi_align_kernel.cu writes them, unfused and with start + p * bin fused."""
    p = torch.arange(n_bins, dtype=torch.float32)[None, :, None]
    i = torch.arange(sn, dtype=torch.float32)[None, None, :]
    s, b = start[:, None, None], bins[:, None, None]
    off = _f32((i + off_frac) * b) / float(sn)
    base_u = _f32(p * b) + s
    base_f = _f32(s.double() + p.double() * b.double())
    return base_u + off, base_f + off


def roi_geometry(rois, spatial_scale, sample_num, PH, PW):
    """roi_geom in f32: (batch, start_w, start_h, bin_w, bin_h, sn_h, sn_w) per roi."""
    r = rois.float()
    sc = torch.tensor(spatial_scale, dtype=torch.float32)
    start_w, start_h = r[:, 1] * sc, r[:, 2] * sc
    end_w, end_h = (r[:, 3] + 1.0) * sc, (r[:, 4] + 1.0) * sc
    roi_w, roi_h = (end_w - start_w).clamp(min=0.0), (end_h - start_h).clamp(min=0.0)
    bin_h, bin_w = roi_h / float(PH), roi_w / float(PW)
    if sample_num > 0:
        sn_h = torch.full_like(r[:, 0], sample_num).long()
        sn_w = sn_h.clone()
    else:
        sn_h, sn_w = torch.ceil(roi_h / float(PH)).long(), torch.ceil(roi_w / float(PW)).long()
    return r[:, 0].long(), start_w, start_h, bin_w, bin_h, sn_h, sn_w


def roi_align_matrix(rois, B, H, W, PH, PW, spatial_scale, sample_num, off_frac=0.5, border_mut=False):
    """The interpolation matrix of RoIAlign (see the module docstring).  off_frac / border_mut exist only to state plausible kernel
    mistakes (sample offset i * bin / sn instead of (i + 1/2) * bin / sn; the window (-1, size - 1] instead of (-1, size])."""
    rois = rois.detach().cpu()
    K = rois.shape[0]
    batch, start_w, start_h, bin_w, bin_h, sn_h, sn_w = roi_geometry(rois, spatial_scale, sample_num, PH, PW)
    A = RoiMatrix(K * PH * PW, B * H * W)
    A.sn_h, A.sn_w = sn_h, sn_w
    keys = torch.stack([sn_h, sn_w], 1)
    for key in torch.unique(keys, dim=0).tolist():
        sh, sw = key
        ks = torch.nonzero((keys[:, 0] == sh) & (keys[:, 1] == sw)).flatten()
        if sh == 0 or sw == 0 or ks.numel() == 0:
            continue                                         # no samples: the bin reads nothing (forward 0 / 0, backward nothing)
        yu, yf = _coords(start_h[ks], bin_h[ks], PH, sh, off_frac)     # [k, PH, sh]
        xu, xf = _coords(start_w[ks], bin_w[ks], PW, sw, off_frac)     # [k, PW, sw]
        ylo, yhi, ywl, ywh, yok = _axis(yu, H, border_mut)
        xlo, xhi, xwl, xwh, xok = _axis(xu, W, border_mut)
        ny, nx = PW * sw, PH * sh                          # each y sample meets PW * sw x samples, and the other way round
        st = A.stats
        st['y_neg'] += int(((yu > -1) & (yu <= 0)).sum()) * ny
        st['x_neg'] += int(((xu > -1) & (xu <= 0)).sum()) * nx
        st['y_clamped'] += int((yok & (yu >= H - 1)).sum()) * ny
        st['x_clamped'] += int((xok & (xu >= W - 1)).sum()) * nx
        yl, xl = yok.sum((1, 2)), xok.sum((1, 2))           # per roi: live samples per axis
        st['live'] += int((yl * xl).sum())
        st['y_dead_only'] += int(((PH * sh - yl) * xl).sum())
        st['x_dead_only'] += int((yl * (PW * sw - xl)).sum())
        st['dead'] += int((PH * sh * PW * sw - yl * xl).sum())
        if sh == 2 and sw == 2:
            my = _merges(ylo, yhi, ywl, ywh, yok)          # [k, PH]
            mx = _merges(xlo, xhi, xwl, xwh, xok)          # [k, PW]
            A.merging_bins += int((my[:, :, None] | mx[:, None, :]).sum())
        # a fused coordinate must not cross the (-1, size] window: there a tap appears or vanishes, no Lipschitz bound holds
        assert torch.equal(_axis(yf, H, border_mut)[4], yok) and torch.equal(_axis(xf, W, border_mut)[4], xok), \
            'a sample lies within one rounding of the window edge: move the roi'
        ey, ex = (yf.double() - yu.double()).abs(), (xf.double() - xu.double()).abs()
        k = ks.numel()
        cnt = float(sh * sw)
        # broadcast to [k, PH, PW, sh, sw]
        Y = lambda t: t[:, :, None, :, None]
        X = lambda t: t[:, None, :, None, :]
        ok = (Y(yok) & X(xok)).double()
        rowi = (ks[:, None, None] * PH * PW + torch.arange(PH)[None, :, None] * PW + torch.arange(PW)[None, None, :])[:, :, :, None, None]
        bb = batch[ks][:, None, None, None, None]
        e = (Y(ey) + X(ex)) * ok / cnt
        shape = (k, PH, PW, sh, sw)
        for yi, wy in ((ylo, ywl), (yhi, ywh)):
            for xi, wx in ((xlo, xwl), (xhi, xwh)):
                col = (bb * H + Y(yi)) * W + X(xi)
                A.row.append(rowi.expand(shape).reshape(-1))
                A.col.append(col.expand(shape).reshape(-1))
                A.val.append((Y(wy) * X(wx) * ok / cnt).expand(shape).reshape(-1))
                A.eps.append(e.expand(shape).reshape(-1))
    return A.finish()


def _chunks(n, step):
    for a in range(0, n, step):
        yield a, min(n, a + step)


def apply_T(A, G, absolute=False, chunk_elems=1 << 26):
    """A^T G in f64 for G [rows, C] (any float dtype, any device A lives on) -> [cols, C] f64; absolute: |A|^T |G|."""
    C = G.shape[1]
    out = torch.zeros((A.cols, C), dtype=torch.float64, device=G.device)
    step = max(1, chunk_elems // max(C, 1))
    for a, b in _chunks(A.row.numel(), step):
        g = G.index_select(0, A.row[a:b]).double()
        if absolute:
            g = g.abs()
        out.index_add_(0, A.col[a:b], g * A.val[a:b, None])
    return out


def apply(A, F, absolute=False, weights=None, chunk_elems=1 << 26):
    """A F in f64 for F [cols, C] -> [rows, C]; weights overrides A's values (e.g. A.eps)."""
    C = F.shape[1]
    val = A.val if weights is None else weights
    out = torch.zeros((A.rows, C), dtype=torch.float64, device=F.device)
    step = max(1, chunk_elems // max(C, 1))
    for a, b in _chunks(A.row.numel(), step):
        f = F.index_select(0, A.col[a:b]).double()
        if absolute:
            f = f.abs()
        out.index_add_(0, A.row[a:b], f * val[a:b, None])
    return out


def apply_T_eps(A, G):
    """E^T |G|: the coordinate-rounding allowance of the backward (zero where no fused coordinate differs)."""
    sel = torch.nonzero(A.eps > 0).flatten()
    out = torch.zeros((A.cols, G.shape[1]), dtype=torch.float64, device=G.device)
    if sel.numel():
        out.index_add_(0, A.col[sel], G.index_select(0, A.row[sel]).double().abs() * A.eps[sel, None])
    return out


def roi_backward_bound(A, G):
    """(reference A^T G, per-element bound) for the backward's f32 atomics: C_ROI (n_cell + 4) u (A^T|G|) + E^T|G|."""
    ref = apply_T(A, G)
    n = A.n_cell().to(G.device).double()[:, None]
    tol = C_ROI * (n + 4.0) * U * apply_T(A, G, absolute=True) + apply_T_eps(A, G)
    return ref, tol


def roi_forward_bound(A, F):
    """(reference A F, per-element bound) for the forward's f32 sums: C_ROI (m + 4) u (A|F|) + E|F|, m = taps of the bin."""
    ref = apply(A, F)
    m = A.n_row().to(F.device).double()[:, None]
    tol = C_ROI * (m + 4.0) * U * apply(A, F, absolute=True) + apply(A, F, absolute=True, weights=A.eps)
    return ref, tol


def merge_path_stats(A, layout_nhwc):
    """Which branch of roi_align_bwd_kernel the bins take: the 2 x 2 merge path (NHWC, sn_h == sn_w == 2) or the general loop;
    and of the merge-path bins, how many merge taps (two of a bin's row taps in one feature row, or two column taps in one
    column: what the merge was written for, bins under two cells).  -> dict(merge_bins, merging_bins, general_bins)."""
    two = int(((A.sn_h == 2) & (A.sn_w == 2)).sum()) * (A.rows // max(1, A.sn_h.numel()))
    if not layout_nhwc:
        return dict(merge_bins=0, merging_bins=0, general_bins=A.rows)
    return dict(merge_bins=two, merging_bins=A.merging_bins, general_bins=A.rows - two)


def _merges(lo, hi, wl, wh, ok):
    """[..., 2] axis taps of the two samples of a bin -> [...] True where two taps with non-zero weight share a row (column)."""
    idx = torch.cat([lo, hi], -1)
    w = torch.cat([wl, wh], -1) * ok.double().repeat(*([1] * (ok.dim() - 1)), 2)
    live = w != 0
    same = (idx[..., :, None] == idx[..., None, :]) & live[..., :, None] & live[..., None, :]
    return same.sum((-1, -2)) > live.sum(-1)


def roi_cases(B, H, W, n, seed, stride=16.0):
    """Random RoIs over B frames (image = map x stride) plus the special ones of the parity suite's _roi_cases: the full image, a
    single pixel, a malformed box (x2 < x1), boxes sticking out top-left and bottom-right, one fully outside; sizes from well under
    one cell per bin (7 x 7 bins: boxes under 7 cells) to the whole map."""
    g = torch.Generator().manual_seed(seed)
    iw, ih = W * stride, H * stride
    xy = torch.rand((n, 2), generator=g) * torch.tensor([iw, ih])
    wh = torch.exp(torch.rand((n, 2), generator=g) * math.log(ih)) + 1        # log-uniform 1 .. image height px
    rois = torch.cat([torch.randint(0, B, (n, 1), generator=g).float(), xy, xy + wh], 1)
    rois[0, 1:] = torch.tensor([0., 0., iw - 1, ih - 1])
    rois[1, 1:] = torch.tensor([50., 60., 50., 60.])
    rois[2, 1:] = torch.tensor([120., 90., 40., 30.])
    rois[3, 1:] = torch.tensor([-200., -150., 80., 60.])
    rois[4, 1:] = torch.tensor([iw - 40, ih - 30, iw + 300, ih + 200])
    rois[5, 1:] = torch.tensor([iw + 50, ih + 50, iw + 90, ih + 90])
    return rois


def edge_rois(B, H, W, stride=16.0):
    """Hand-placed RoIs for the border rules of make_tap (spatial scale 1 / stride, 7 x 7 bins): bins under one cell, of one to
    two cells, samples on the clamped last row / column, samples in (-1, 0], samples outside on one axis only, zero width."""
    s = stride
    iw, ih = W * s, H * s
    out = []
    for b in range(B):
        out += [
            [b, 3.3 * s, 2.1 * s, 3.3 * s + 40, 2.1 * s + 50],               # 7 x 7 bins inside a 3 x 4 cell box: bins << one cell
            [b, 5.0 * s, 4.0 * s, 5.0 * s + 7 * 16 * 1.5, 4.0 * s + 7 * 16 * 1.2],   # bins of 1.2 - 1.5 cells
            [b, 2.0 * s, 1.0 * s, 2.0 * s + 7 * 16 * 1.9, 1.0 * s + 7 * 16 * 1.7],   # bins of 1.7 - 1.9 cells
            [b, iw - 3.2 * s, ih - 2.6 * s, iw - 0.5 * s, ih - 0.2 * s],      # samples on the clamped last row and column
            [b, iw - 1.4 * s, ih - 1.1 * s, iw + 0.9 * s, ih + 0.3 * s],      # samples in (H - 1, H] and past it
            [b, -0.9 * s, -0.6 * s, 2.5 * s, 1.7 * s],                         # samples in (-1, 0]
            [b, -0.95 * s, 3.0 * s, 0.5 * s, 6.0 * s],                         # (-1, 0] in x only
            [b, 4.0 * s, -3.0 * s, 9.0 * s, 2.0 * s],                          # outside in y only (top rows of bins dead)
            [b, iw - 2.0 * s, 5.0 * s, iw + 6.0 * s, 9.0 * s],                 # outside in x only (right columns dead)
            [b, 7.5 * s, 6.5 * s, 7.5 * s - 1, 6.5 * s + 30],                  # zero width (x2 + 1 == x1)
            [b, 9.0 * s, 3.0 * s, 9.0 * s, 3.0 * s],                           # one pixel
        ]
    return torch.tensor(out, dtype=torch.float32)


def adaptive_rois(B, H, W, stride=16.0, seed=3):
    """sample_num = 0: RoIs whose adaptive grid (ceil(extent / 7 cells)) is 2 x 2 (the merge path in NHWC) next to 1 x 1, 1 x 2,
    2 x 1 and 3 x 3 (the general loop)."""
    g = torch.Generator().manual_seed(seed)
    s = stride
    out = []
    for (gh, gw) in ((2, 2), (1, 1), (1, 2), (2, 1), (3, 3), (2, 2), (1, 3)):
        for _ in range(3):
            eh = (gh - 1 + 0.2 + 0.7 * float(torch.rand((), generator=g))) * 7.0        # extent in cells: ceil(e / 7) == gh
            ew = (gw - 1 + 0.2 + 0.7 * float(torch.rand((), generator=g))) * 7.0
            y0 = float(torch.rand((), generator=g)) * max(0.5, H - eh) - 0.5
            x0 = float(torch.rand((), generator=g)) * max(0.5, W - ew) - 0.5
            b = int(torch.randint(0, B, (1,), generator=g))
            out.append([b, x0 * s, y0 * s, (x0 + ew) * s - 1, (y0 + eh) * s - 1])
    return torch.tensor(out, dtype=torch.float32)


# ------------------------------------------------------------------------------- colsum (hvr_colsum)
def colsum_slices(M, N):
    """misc.hip colsum_slices: ~1 024 workgroups of 64 columns, at least 16 rows per row lane, at most 256 slices."""
    cols = (N + 63) // 64
    s = (1024 + cols - 1) // cols
    s = min(s, (M + 63) // 64)
    return max(1, min(256, s))


def colsum_chain(M, N):
    """Longest chain of f32 additions behind one column sum: a row lane adds ceil(M / 4S) rows (the first onto 0 is exact), two
    levels join the four lanes, and S > 1 partials are added by the second kernel."""
    S = colsum_slices(M, N)
    per_lane = -(-M // (4 * S))
    return (per_lane - 1) + 2 + (S - 1 if S > 1 else 0)


def colsum_bound(x):
    """(f64 column sums, per-column bound (chain + 1) u sum|x|) of x [M, N] (any float dtype; any device)."""
    M, N = x.shape
    xd = x.double()
    return xd.sum(0), (colsum_chain(M, N) + 1) * U * xd.abs().sum(0)


def colsum_emulated(x, slice_start=4):
    """The kernel's summation order in f32 on the host (row lane r0 of slice y: rows slice_start * y + r0, stride 4 S), for stating
    a slice-indexing mistake (slice_start = 1: slice y starts at row y)."""
    M, N = x.shape
    S = colsum_slices(M, N)
    xf = x.float()
    parts = []
    for y in range(S):
        lanes = []
        for r0 in range(4):
            rows = torch.arange(slice_start * y + r0, M, 4 * S)
            lanes.append(xf[rows].sum(0) if rows.numel() else torch.zeros(N))
        parts.append((lanes[0] + lanes[1]) + (lanes[2] + lanes[3]))
    return torch.stack(parts).sum(0)


# ------------------------------------------------------------------------------- weight pack / unpack
def pack_statement(w, s, dtype):
    """pack_conv_weight: (w * s) permuted to [Cout][KH][KW][Cin], rounded once to dtype."""
    return (w * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).to(dtype)


def pack_groups(shapes, firsts, eff_bytes_mod16):
    """Branch of every 8-element group of pack_conv_weights_multi_kernel: (fast, elementwise, straddling) counts, from its rule
    (Cin % 8 == 0, group start 8-aligned within the item, group inside the item, output 16-byte aligned)."""
    total = firsts[-1] + math.prod(shapes[-1])
    fast = slow = straddle = 0
    item = 0
    for v in range((total + 7) // 8):
        idx = v * 8
        while item + 1 < len(firsts) and firsts[item + 1] <= idx:
            item += 1
        Cout, Cin, KK = shapes[item]
        e, n = idx - firsts[item], Cout * Cin * KK
        if Cin % 8 == 0 and e % 8 == 0 and e + 8 <= n and eff_bytes_mod16[item] == 0:
            fast += 1
        else:
            slow += 1
            straddle += int(e + 8 > n and idx + 8 <= total)
    return fast, slow, straddle


def pack_flat(ws, ss, firsts, dtype, straddle_uses_first_item=False):
    """The flat work list of pack_conv_weights_multi (item i at firsts[i]), element by element, on the host.
    straddle_uses_first_item states a plausible mistake: the elements of a group of eight that straddles two items decomposed
    with the Cin / KK of the item the group starts in (indices wrapped into the right item's weight)."""
    total = firsts[-1] + ws[-1].numel()
    fi = torch.tensor(firsts)
    idx = torch.arange(total)
    item = torch.searchsorted(fi, idx, right=True) - 1
    dec = torch.searchsorted(fi, idx // 8 * 8, right=True) - 1 if straddle_uses_first_item else item
    out = torch.empty(total, dtype=dtype)
    for i, (w, s) in enumerate(zip(ws, ss)):
        sel = torch.nonzero(item == i).flatten()
        e = sel - firsts[i]
        Cout, Cin, KH, KW = w.shape
        cin = torch.tensor([ws[j].shape[1] for j in range(len(ws))])[dec[sel]]
        kk = torch.tensor([ws[j].shape[2] * ws[j].shape[3] for j in range(len(ws))])[dec[sel]]
        c, r = e % cin, e // cin
        t, o = r % kk, r // kk
        o, c, t = o % Cout, c % Cin, t % (KH * KW)
        wf = w.reshape(Cout, Cin, KH * KW)
        out[sel] = (wf[o, c, t] * s[o]).to(dtype)
    return out


def fma_f32(a, s, d):
    """fma(a, s, d) in f32, stated without any f32 fused multiply-add: a * s is exact in f64 and a * s + d is rounded in f64 once;
    rounding that to f32 (double rounding) is wrong only where the f64 sum lands exactly on an f32 midpoint while the exact sum
    does not (its TwoSum error is non-zero): there the exact sum's side decides.
    -> (correctly rounded f32, mask where f64-then-f32 could double-round, mask where it actually does)."""
    p = a.double() * s.double()
    dd = d.double()
    t = p + dd
    bv = t - p
    err = (p - (t - bv)) + (dd - bv)                    # TwoSum: t + err == a * s + d exactly
    r = t.float()
    inf = torch.full_like(r, float('inf'))
    below = torch.where(r.double() > t, torch.nextafter(r, -inf), r)
    above = torch.nextafter(below, inf)
    risky = ((below.double() + above.double()) / 2 == t) & (err != 0)
    exact = torch.where(risky, torch.where(err > 0, above, below), r)
    return exact, risky, risky & (exact != r)


def unpack_groups(shapes, firsts, out_addr_mod16):
    """Branch of every 4-element group of unpack_conv_wgrads_multi_kernel, from its rule (group inside the item, its first output
    16-byte aligned): -> (vector, elementwise, straddling) counts.  out_addr_mod16[i]: byte address of item i's output mod 16."""
    total = firsts[-1] + math.prod(shapes[-1])
    vec = slow = straddle = 0
    item = 0
    for v in range((total + 3) // 4):
        idx = v * 4
        while item + 1 < len(firsts) and firsts[item + 1] <= idx:
            item += 1
        e, n = idx - firsts[item], math.prod(shapes[item])
        if e + 4 <= n and (out_addr_mod16[item] + 4 * e) % 16 == 0:
            vec += 1
        else:
            slow += 1
            straddle += int(e + 4 > n and idx + 4 <= total)
    return vec, slow, straddle
