"""Plain float64 statement of deformable RoI pooling (hvr_deform_roi_pool_fwd, the pooling of DCN v1 / v2), written from the rule the
C ABI states (include/hvr_hip.h) independently of the HIP code, with the error bound that tests/test_dpool_refs.py (CPU) and
tests/test_dpool_gpu.py (GPU) hold the kernel to.  Style and constants of tests/dcn_refs.py.

The rule.  feat [B, H, W, C] (stored values), rois [K, 5] f32, trans [K, ncls 2 ps ps] f32 or None, mask_logit [K, P P] f32 or None.
The POSITION CHAIN is evaluated in torch f32 on the CPU, one torch operation per f32 operation of the rule, in the rule's order:
    rnd (half away from zero), start = rnd(x1) s - 0.5, end = (rnd(x2) + 1) s - 0.5, roi = max(end - start, f32(0.1)), bin = roi / P,
    sub = bin / spp, part = floor(float(p) / P ps), t = trans[part] trans_std, start_bin = (float(p) bin + start) + t roi,
    pos = start_bin + float(i) sub, the skip test at -0.5 / size - 0.5, the clamp to [0, size - 1], floor and ceil.
That is the only f32 part: positions, validity and corner cells are then the kernel's own.  Everything from dx = pos - floor(pos),
dy on is float64: the weights, the four products, the sum over the samples inside, the division by their count and the sigmoid.

Bound on the f32 value the kernel holds before its store, per element: c u sum |weight| |value| / count (. mask), first order,
times SECOND.  c counts the f32 roundings behind one term of the sum when no operation is fused (-ffp-contract=off):
    C_ONE_MINUS = 2   1 - dx and 1 - dy            (dx, dy themselves are exact: pos and floor(pos) are f32 numbers, pos >= 0)
    C_WEIGHT = 1      the weight product
    C_PRODUCT = 1     weight . value
    C_ADDS = 3        three additions join a sample's four products
    spp^2 - 1         additions across the samples of a bin (the first lands on 0)
    C_DIVIDE = 1      sum / count (count is an exact small integer)
  c = spp^2 + 7; modulated: C_MASK = 1 for the product and S_SIGMOID (dcn_refs: expf of EXPF_ULP ulp, a correctly rounded add and
  divide) for the mask itself.  No bound contains a value measured on a device.

Stored output: bf16 / half: ONE rounding of the f32 value; split half: the SPLIT_REL / SPLIT_ABS rule; f32: the bound itself
(forward_kernel_refs.stored_bracket, which goes through train_loss_refs.bracket).

`mistake=`: plausible kernel mistakes stated exactly (MISTAKES); tests/test_dpool_refs.py shows each outside the bound on the random
cases or unequal on an exact family.
"""
import torch

from tests import dcn_refs as D
from tests import forward_kernel_refs as F
from tests import train_loss_refs as L

U = L.U
SECOND = L.SECOND
C_ONE_MINUS, C_WEIGHT, C_PRODUCT, C_ADDS, C_DIVIDE, C_MASK = 2, 1, 1, 3, 1, 1
S_SIGMOID = D.S_SIGMOID
SENTINEL = F.SENTINEL

MISTAKES = ('round_half_even', 'no_half_shift', 'min_size_zero', 'roialign_border', 'no_edge_clamp', 'divide_by_spp2', 'trans_by_bin',
            'trans_xy_swapped', 'trans_unscaled', 'mask_by_part', 'mask_unapplied', 'group_ignored', 'batch_ignored')


def roundings(spp, modulated):
    return C_ONE_MINUS + C_WEIGHT + C_PRODUCT + C_ADDS + (spp * spp - 1) + C_DIVIDE + ((C_MASK + S_SIGMOID) if modulated else 0)


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def rnd(x, mistake=None):
    """C roundf on f32 numbers: half AWAY from zero (in f64: |x| + 0.5 is exact there; in f32 it is not, 0.49999997 + 0.5 = 1)."""
    if mistake == 'round_half_even':
        return torch.round(x)
    xd = x.double()
    return (torch.sign(xd) * torch.floor(xd.abs() + 0.5)).float()


def pool_statement(feat, rois, trans, mask_logit, P, out_channels, group_size, part_size, sample_per_part, spatial_scale, trans_std,
                   mistake=None, info=False):
    """feat [B, H, W, C] true stored values (any float dtype), rois [K, 5], trans [K, ncls 2 ps ps] f32 or None, mask_logit [K, P P]
    f32 or None (both possibly column slices) -> (ref, bound) f64 [K, P, P, out_channels], the bound on the f32 value before the
    store; info=True appends the per-(roi, class, bin) count of samples inside [K, ncls, P, P].  Runs on the CPU.  Mistakes:
      round_half_even   the roi corners rounded half to even (torch.round, rintf) instead of half away from zero (roundf)
      no_half_shift     start and end without the - 0.5
      min_size_zero     roi size max(end - start, 0) as RoIAlign
      roialign_border   a sample skipped outside [-1, size] (RoIAlign's test) instead of [-0.5, size - 0.5]
      no_edge_clamp     no clamp to [0, size - 1]: a corner cell outside the map contributes 0
      divide_by_spp2    the sum divided by spp^2 whatever the count
      trans_by_bin      the offset read at [min(ph, ps - 1)][min(pw, ps - 1)] instead of [part_h][part_w]
      trans_xy_swapped  x offset from channel 1, y offset from channel 0
      trans_unscaled    trans_std dropped
      mask_by_part      the mask logit read at [part_h][part_w] of its P x P grid
      mask_unapplied    the mask never multiplied in
      group_ignored     channel (ct gs + 0) gs + 0 for every bin
      batch_ignored     every roi pooled from frame 0"""
    assert mistake is None or mistake in MISTAKES, mistake
    x = feat.detach().cpu().double()
    rois = rois.detach().cpu().float()
    B, H, W, C = x.shape
    K = rois.shape[0]
    Cout, gs, ps, spp = int(out_channels), int(group_size), int(part_size), int(sample_per_part)
    assert C == Cout * gs * gs
    ncls = 1
    if trans is not None:
        trans = trans.detach().cpu().float()
        assert trans.shape[0] == K and trans.shape[1] % (2 * ps * ps) == 0
        ncls = trans.shape[1] // (2 * ps * ps)
        trans = trans.reshape(K, ncls, 2, ps, ps)
    assert Cout % ncls == 0
    cpc = Cout // ncls
    s, Pf, sppf, psf, gsf, half = _f32(spatial_scale), _f32(P), _f32(spp), _f32(ps), _f32(gs), _f32(0.5)
    tstd = _f32(1.0 if mistake == 'trans_unscaled' else trans_std)
    shift = _f32(0.0) if mistake == 'no_half_shift' else half
    floor_min = _f32(0.0 if mistake == 'min_size_zero' else 0.1)
    idx = torch.arange(P)
    pf = idx.float()
    part = torch.floor(pf / Pf * psf).long()                         # [P]
    assert int(part.min()) >= 0 and int(part.max()) <= ps - 1
    grp = torch.floor(pf * gsf / Pf).long().clamp(0, gs - 1)          # [P]
    tpart = idx.clamp(max=ps - 1) if mistake == 'trans_by_bin' else part
    cx, cy = (1, 0) if mistake == 'trans_xy_swapped' else (0, 1)

    def axis(c1, c2, size, ch, along_w):
        """-> (ok, lo, hi, d, 1 - d as f64) each [K, ncls, P(ph), P(pw), spp]"""
        start = rnd(rois[:, c1], mistake) * s - shift                # [K]
        end = (rnd(rois[:, c2], mistake) + _f32(1.0)) * s - shift
        roi = torch.maximum(end - start, floor_min)
        bin_ = roi / Pf
        sub = bin_ / sppf
        if trans is None:
            t = torch.zeros((K, 1, P, P), dtype=torch.float32)
        else:
            t = trans[:, :, ch][:, :, tpart][:, :, :, tpart] * tstd  # [K, ncls, ph, pw]
        p_ax = pf.view(1, 1, 1, P) if along_w else pf.view(1, 1, P, 1)
        v = lambda a: a.view(K, 1, 1, 1)
        st = p_ax * v(bin_) + v(start)
        st = st + t * v(roi)
        pos = st[..., None] + torch.arange(spp).float() * v(sub)[..., None]      # [K, ncls, P, P, spp]
        if mistake == 'roialign_border':
            ok = ~((pos < -1.0) | (pos > float(size)))
        else:
            ok = ~((pos < -0.5) | (pos > _f32(size) - half))
        if mistake != 'no_edge_clamp':
            pos = pos.clamp(0.0, float(size - 1))
        lo, hi = torch.floor(pos), torch.ceil(pos)
        d = pos.double() - lo.double()
        return ok, lo.long(), hi.long(), d

    okw, xl, xh, dx = axis(1, 3, W, cx, True)
    okh, yl, yh, dy = axis(2, 4, H, cy, False)
    nc = okw.shape[1]
    bi = rois[:, 0].long().clamp(0, B - 1)
    if mistake == 'batch_ignored':
        bi = torch.zeros_like(bi)
    bi = bi.view(K, 1, 1, 1)
    gh, gw = grp.view(1, P, 1, 1), grp.view(1, 1, P, 1)
    if mistake == 'group_ignored':
        gh, gw = torch.zeros_like(gh), torch.zeros_like(gw)
    ref = torch.zeros((K, P, P, Cout), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    counts = torch.zeros((K, ncls, P, P), dtype=torch.long)
    for cls in range(ncls):
        cl = cls if nc > 1 else 0
        ct = torch.arange(cls * cpc, (cls + 1) * cpc).view(1, 1, 1, cpc)
        cidx = (ct * gs + gh) * gs + gw                                        # [1, P, P, cpc]
        acc = torch.zeros((K, P, P, cpc), dtype=torch.float64)
        m = torch.zeros_like(acc)
        cnt = torch.zeros((K, P, P), dtype=torch.long)
        for ih in range(spp):
            for iw in range(spp):
                ok = okh[:, cl, :, :, ih] & okw[:, cl, :, :, iw]               # [K, P, P]
                ax, ay = dx[:, cl, :, :, iw][..., None], dy[:, cl, :, :, ih][..., None]
                val = torch.zeros_like(acc)
                mv = torch.zeros_like(acc)
                for (yy, xx, wgt) in ((yl, xl, (1 - ax) * (1 - ay)), (yh, xl, (1 - ax) * ay), (yl, xh, ax * (1 - ay)), (yh, xh, ax * ay)):
                    yi, xi = yy[:, cl, :, :, ih][..., None], xx[:, cl, :, :, iw][..., None]
                    inmap = (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)  # (always true unless 'no_edge_clamp')
                    v = x[bi, yi.clamp(0, H - 1), xi.clamp(0, W - 1), cidx] * inmap
                    val = val + wgt * v
                    mv = mv + wgt.abs() * v.abs()
                acc = acc + val * ok[..., None]
                m = m + mv * ok[..., None]
                cnt = cnt + ok.long()
        counts[:, cls] = cnt
        div = torch.full_like(cnt, spp * spp) if mistake == 'divide_by_spp2' else cnt
        div = div.clamp(min=1).double()[..., None]
        nz = (cnt > 0)[..., None]
        ref[..., cls * cpc:(cls + 1) * cpc] = acc / div * nz
        mag[..., cls * cpc:(cls + 1) * cpc] = m / div * nz
    modulated = mask_logit is not None
    if modulated and mistake != 'mask_unapplied':
        ml = mask_logit.detach().cpu().float().reshape(K, -1)
        assert ml.shape[1] == P * P
        ml = ml.reshape(K, P, P)
        if mistake == 'mask_by_part':
            ml = ml[:, part][:, :, part]
        mask = torch.sigmoid(ml.double())[..., None]
        ref, mag = ref * mask, mag * mask
    bound = SECOND * roundings(spp, modulated) * U * mag
    return (ref, bound, counts) if info else (ref, bound)


def stored_bracket(ref, bound, mode):
    return F.stored_bracket(ref, bound, mode)


def special_rois(B, H, W, scale):
    """The RoIs every case carries (image units; the map covers [0, W / scale) x [0, H / scale)): the whole map, two wholly off the
    map (beyond the far corner, before the origin), a degenerate one (x2 < x1, y2 < y1), corners on .5 of both signs, and boxes that
    hang over each border."""
    iw, ih = W / scale, H / scale
    r = [
        (0, 0.0, 0.0, iw - 1.0, ih - 1.0),
        (B - 1, iw + 200.0, ih + 200.0, iw + 330.0, ih + 290.0),
        (0, -500.0, -400.0, -300.0, -250.0),
        (B - 1, 0.6 * iw, 0.5 * ih, 0.25 * iw, 0.2 * ih),
        (0, 10.5, 20.5, 0.5 * iw + 0.5, 0.6 * ih + 0.5),
        (B - 1, -10.5, -4.5, 0.4 * iw + 0.5, 0.5 * ih + 0.5),
        (0, -0.45 * iw, -0.35 * ih, 0.35 * iw, 0.45 * ih),
        (B - 1, 0.6 * iw, 0.55 * ih, 1.5 * iw, 1.4 * ih),
        (0, 0.3 * iw, -0.8 * ih, 0.5 * iw, 0.3 * ih),
    ]
    return torch.tensor(r, dtype=torch.float32)


def real_case(mode, seed, B=2, H=9, W=11, out_channels=64, group_size=1, K=40, P=7, spp=4, ps=7, ncls=1, modulated=True, scale=1.0 / 16,
              trans_std=0.1, trans_spread=3.0, ldt=None, ldm=None, check=True, pick=None):
    """Real-statistics inputs: a map after a ReLU rounded to what `mode` stores (f64 true values), the special RoIs above plus random
    ones (centres anywhere on the image, sides up to 0.9 of it, corners on a grid of 1/4 so that .5 and .25 occur), offsets
    N(0, trans_spread) (trans_std 0.1: a bin moves by up to the roi's own size, samples leave the map), mask logits N(0, 2).  trans
    / mask_logit come as column slices of wider buffers when ldt / ldm are given (filler 1000 in the unused columns).  check: assert
    that the case contains what a test must not miss (see _assert_coverage).  pick: the indices of the special RoIs to carry when K is
    smaller than their number (then check must be off).  -> dict."""
    g = torch.Generator().manual_seed(seed)
    C = out_channels * group_size * group_size
    feat = F.store_true(torch.randn((B, H, W, C), generator=g).clamp(min=0.0), mode, 'act')
    sp = special_rois(B, H, W, scale)
    if pick is not None:
        assert not check
        sp = sp[torch.tensor(pick)]
    assert K >= sp.shape[0]
    n = K - sp.shape[0]
    iw, ih = W / scale, H / scale
    cxy = torch.rand((n, 2), generator=g) * torch.tensor([iw, ih])
    wh = (torch.rand((n, 2), generator=g) * 0.9 + 0.02) * torch.tensor([iw, ih])
    box = torch.round(torch.cat([cxy - wh / 2, cxy + wh / 2], 1) * 4) / 4
    bidx = torch.randint(0, B, (n, 1), generator=g).float()
    rois = torch.cat([sp, torch.cat([bidx, box], 1)], 0)
    nt = ncls * 2 * ps * ps
    tbuf = torch.full((K, nt if ldt is None else ldt), 1000.0)
    tbuf[:, :nt] = torch.randn((K, nt), generator=g) * trans_spread
    mbuf = torch.full((K, P * P if ldm is None else ldm), 1000.0)
    mbuf[:, :P * P] = torch.randn((K, P * P), generator=g) * 2.0
    case = dict(feat=feat, rois=rois, trans=tbuf[:, :nt], mask_logit=mbuf[:, :P * P] if modulated else None, trans_buf=tbuf, mask_buf=mbuf,
                P=P, out_channels=out_channels, group_size=group_size, part_size=ps, sample_per_part=spp, spatial_scale=scale,
                trans_std=trans_std, mode=mode)
    if check:
        _assert_coverage(case)
    return case


def args_of(case, trans=True, mask=True):
    """The positional arguments of pool_statement behind (feat, rois)."""
    return (case['trans'] if trans else None, case['mask_logit'] if mask else None, case['P'], case['out_channels'], case['group_size'],
            case['part_size'], case['sample_per_part'], case['spatial_scale'], case['trans_std'])


def _assert_coverage(case):
    """A case must contain: bins with count == 0, bins with 0 < count < spp^2, full bins (with and without offsets); RoIs with .5
    coordinates of both signs; a degenerate RoI; RoIs wholly off the map (every bin empty, without offsets); a RoI covering the whole
    map (every bin full, without offsets) -- otherwise a test built on it could hide a blind spot."""
    rois, spp = case['rois'], case['sample_per_part']
    full = spp * spp
    for with_trans in (False, True):
        _, _, cnt = pool_statement(case['feat'], rois, *args_of(case, trans=with_trans, mask=False), info=True)
        assert bool((cnt == 0).any()) and bool(((cnt > 0) & (cnt < full)).any()) and bool((cnt == full).any()), with_trans
        if not with_trans:
            per_roi = cnt.reshape(cnt.shape[0], -1)
            assert bool((per_roi == 0).all(1).any()), 'no RoI wholly off the map'
            assert bool((per_roi == full).all(1).any()), 'no RoI covering the map'
    xy = rois[:, 1:]
    frac = (xy - torch.floor(xy)) == 0.5
    assert bool((frac & (xy > 0)).any()) and bool((frac & (xy < 0)).any()), 'no .5 coordinates of both signs'
    assert bool(((rois[:, 3] < rois[:, 1]) & (rois[:, 4] < rois[:, 2])).any()), 'no degenerate RoI'
    H, W, sc = case['feat'].shape[1], case['feat'].shape[2], case['spatial_scale']
    assert bool(((rois[:, 1] <= 0) & (rois[:, 2] <= 0) & (rois[:, 3] >= W / sc - 1) & (rois[:, 4] >= H / sc - 1)).any()), 'no whole-map RoI'


EXACT_FAMILIES = ('integer', 'eighths', 'zero', 'outside', 'lo_act')


def exact_case(mode, seed, family, B=2, H=9, W=11, out_channels=64, K=24, P=4, spp=2):
    """Inputs on which every f32 operation of a correct kernel behind the positions is exact, so the stored result must EQUAL
    round-to-nearest of the statement.  Map values are integers of <= 5 bits x 2^-4 (lo_act, split half: up to 13-bit integers, a
    non-zero lo half); spatial_scale 1 and integer roi corners make the roi size an integer N, P spp = 8 the sample step N / 8:
    positions are multiples of 1/8, weights multiples of 1/64; trans_std = 0.5 with offsets on multiples of 1/4 keeps that.  Only
    RoIs whose every bin has a power-of-two count (or none) are kept: the division is exact.  family:
      'integer'   sides N that are multiples of 8, no offsets: every position k + 0.5, weights 1/4 ... (integer-valued map x 2^-4)
      'eighths'   any integer side, offsets on multiples of 1/4, a mask of logits cycling {0, +32, -128}: exactly 0.5, 1 and 0
      'zero'      'eighths' with the offsets given and all zero (equal to no offsets at all)
      'outside'   every RoI wholly outside the map: zeros
      'lo_act'    'eighths' on wide split-half values (the lo plane must be read and written)"""
    assert family in EXACT_FAMILIES and P * spp == 8
    g = torch.Generator().manual_seed(seed)
    top = (2 ** 13 - 1) if family == 'lo_act' else 31
    feat = torch.randint(-top, top + 1, (B, H, W, out_channels), generator=g).double() * 2.0 ** -4
    assert bool((F.store_true(feat.float(), mode, 'act') == feat).all())
    n = 8 * K
    x1 = torch.randint(-6, W + 2, (n,), generator=g).float()
    y1 = torch.randint(-6, H + 2, (n,), generator=g).float()
    if family == 'integer':
        sw, sh = torch.randint(1, 3, (n,), generator=g).float() * 8, torch.randint(1, 3, (n,), generator=g).float() * 8
    else:
        sw, sh = torch.randint(1, W + 6, (n,), generator=g).float(), torch.randint(1, H + 6, (n,), generator=g).float()
    if family == 'outside':
        x1 = x1 + torch.where(torch.arange(n) % 2 == 0, torch.tensor(W + 40.0), torch.tensor(-80.0))
    rois = torch.stack([torch.randint(0, B, (n,), generator=g).float(), x1, y1, x1 + sw - 1, y1 + sh - 1], 1)
    trans = mask = None
    if family in ('eighths', 'lo_act', 'zero'):
        trans = torch.randint(-4, 5, (n, 2 * P * P), generator=g).float() / 4.0
        if family == 'zero':
            trans = torch.zeros_like(trans)
        mask = torch.tensor([0.0, 32.0, -128.0])[torch.randint(0, 3, (n, P * P), generator=g)]
    case = dict(feat=feat, rois=rois, trans=trans, mask_logit=mask, P=P, out_channels=out_channels, group_size=1, part_size=P,
                sample_per_part=spp, spatial_scale=1.0, trans_std=0.5, mode=mode)
    _, _, cnt = pool_statement(feat, rois, *args_of(case), info=True)
    cnt = cnt.reshape(n, -1)
    pow2 = ((cnt & (cnt - 1)) == 0).all(1)                      # (0 counts as one)
    keep = torch.nonzero(pow2)[:K, 0]
    assert keep.numel() == K, (family, int(pow2.sum()))
    case['rois'] = rois[keep].contiguous()
    case['trans'] = None if trans is None else trans[keep].contiguous()
    case['mask_logit'] = None if mask is None else mask[keep].contiguous()
    kept = cnt[keep]
    if family == 'outside':
        assert int(kept.max()) == 0
    else:
        assert bool((kept == spp * spp).any()) and bool(((kept > 0) & (kept < spp * spp)).any())
    return case


def to_device_operand(x, mode, device):
    return D.to_device_operand(x, mode, device)
