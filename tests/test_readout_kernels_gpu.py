"""The geometry kernels between the window path's MFMA calls against the f64 statements of tests/readout_refs.py: RoIAlign forward
(roi_align.hip, all four kernels), the RCNN read-out hvr_det_decode (misc.hip), the proposal decode inside hvr_rpn_proposals (nms.hip,
one-workgroup and chip-wide forms), hvr_box_targets and hvr_max_iou_assign (targets.hip).

Every test states its bound and asserts, from the launcher's documented rule, that the branch it targets ran.  Bounds (u = 2^-24):
  * RoIAlign forward, per element: train_kernel_refs.roi_forward_bound, C_ROI (m + 4) u (A|F|) + E|F|; half storage: the stored value
    lies between T(ref - bound) and T(ref + bound), and equals T(ref) where that bracket is one value (more than 0.9 of the elements);
    the exact family: equality (f32) / the reference rounded once (bf16, f16);
  * decode, encode, IoU, softmax, sigmoid: the per-element bound readout_refs.Val propagates (one u per f32 operation, the unfused
    form of a multiply-add, expf / logf at the 3 ulp of the OpenCL C full profile, correctly rounded division);
  * indices, counts, labels, weights, untouched rows: equality.
Every comparison prints `RATIO <call> <mode> <worst error / bound>` (pytest -s); a ratio above 1 fails, and the message names the worst
element and how many elements are over."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hvrnet_amd import native, ops  # noqa: E402
from tests import forward_kernel_refs as FK  # noqa: E402
from tests import readout_refs as R  # noqa: E402
from tests import train_kernel_refs as T  # noqa: E402

DEV = 'cuda:0'
SENT = -768.0            # an f32, bf16 and f16 number no test produces
GUARD_ROWS = 64
NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16', native.SPLIT: 'f16x2'}
NHWC, NCHW = native.LAYOUT_NHWC, native.LAYOUT_NCHW


def _report(what, mode, got, val, extra=''):
    worst, at, nbad = R.ratio(got, val)
    print('RATIO %s %s %.4g' % (what, mode, worst))
    assert worst <= 1.0, '%s %s: %d of %d elements over the bound; worst ratio %g at flat index %d (got %r, statement %r, bound %g) %s' % (
        what, mode, nbad, val.v.numel(), worst, at, float(got.flatten()[at]), float(val.v.flatten()[at]), float(val.e.flatten()[at]), extra)
    return worst


def _dev(val):
    return R.Val(val.v.to(DEV), val.e.to(DEV))


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).to(dtype)


# =============================================================================== RoIAlign forward
_CACHE = {}


def _family(sn):
    """(rois on the device, A on the device) of the forward family, built once per sample_num and left unchanged."""
    if sn not in _CACHE:
        rois = R.roi_family()
        A = T.roi_align_matrix(rois, R.MAP_B, R.MAP_H, R.MAP_W, R.PH, R.PW, R.SCALE, sn)
        for k in ('y_neg', 'x_neg', 'y_clamped', 'x_clamped', 'y_dead_only', 'x_dead_only', 'live'):
            assert A.stats[k] > 0, (k, A.stats)
        _CACHE[sn] = (rois.to(DEV), A.to(DEV), R.nan_rows(A).to(DEV))
    return _CACHE[sn]


def _features(C, dtype, seed, offset=0):
    """[B, H, W, C] maps in dtype; offset: the view starts `offset` elements into a larger buffer."""
    n = R.MAP_B * R.MAP_H * R.MAP_W * C
    flat = torch.zeros(n + offset, dtype=dtype, device=DEV)
    flat[offset:] = _randn((n,), seed, dtype)
    return flat[offset:].view(R.MAP_B, R.MAP_H, R.MAP_W, C)


def _fwd_rows(feat_nhwc, rois, ph, pw, sn, layout):
    """native.roi_align_fwd into a sentinel-filled buffer with GUARD_ROWS rows behind the output; the guards must be intact.
    feat_nhwc: [B, H, W, C] (transposed here for NCHW).  -> rows [K * ph * pw, C] in (roi, ph, pw) order."""
    K, C = rois.shape[0], feat_nhwc.shape[-1]
    n = K * ph * pw * C
    buf = torch.full((n + GUARD_ROWS * C,), SENT, dtype=feat_nhwc.dtype, device=DEV)
    if layout == NHWC:
        out = native.roi_align_fwd(feat_nhwc, rois, ph, pw, R.SCALE, sn, NHWC, out=buf[:n].view(K, ph, pw, C))
        rows = out.reshape(-1, C)
    else:
        out = native.roi_align_fwd(feat_nhwc.permute(0, 3, 1, 2).contiguous(), rois, ph, pw, R.SCALE, sn, NCHW, out=buf[:n].view(K, C, ph, pw))
        rows = out.permute(0, 2, 3, 1).reshape(-1, C)
    assert bool((buf[n:] == SENT).all()), 'guard rows overwritten'
    return rows


def _check_rows(what, got, ref, tol, nan, dtype):
    """got rows against (ref, tol): NaN exactly on `nan` rows; f32 within tol; half types through the bracket."""
    mode = NAMES[dtype]
    isn = torch.isnan(got)
    assert torch.equal(isn.any(1), nan) and torch.equal(isn.all(1), nan), 'NaN rows differ from the bins without samples'
    keep = ~nan
    got, ref, tol = got[keep], ref[keep], tol[keep]
    if dtype == torch.float32:
        return _report(what, mode, got, R.Val(ref, tol))
    lo, hi = (ref - tol).float().to(dtype), (ref + tol).float().to(dtype)
    half = torch.maximum((hi.double() - ref).abs(), (lo.double() - ref).abs())
    worst = _report(what, mode, got, R.Val(ref, half))
    assert bool(((got >= lo) & (got <= hi)).all())
    pinned = lo == hi
    assert float(pinned.double().mean()) > 0.9 and torch.equal(got[pinned], ref.float().to(dtype)[pinned])
    return worst


NHWC_CASES = [(torch.float32, C, sn, 0, 'nhwc<float,4>') for C in (8, 12, 64, 1024) for sn in (2, 0)]
for _dt in (torch.bfloat16, torch.float16):
    NHWC_CASES += [(_dt, C, 2, 0, 'nhwc_bf16_s2') for C in (8, 64, 1024, 2048)]
    NHWC_CASES += [(_dt, 64, sn, 0, 'nhwc<T,8>') for sn in (0, 3)]
    NHWC_CASES += [(_dt, C, 2, 0, 'nhwc<T,4>') for C in (24, 40)]
NHWC_CASES += [(torch.bfloat16, 64, 2, 4, 'nhwc<T,8>')]


@pytest.mark.parametrize('dtype,C,sn,offset,kernel', NHWC_CASES, ids=lambda v: NAMES.get(v, str(v)) if isinstance(v, torch.dtype) else str(v))
def test_roi_align_forward_nhwc(dtype, C, sn, offset, kernel):
    """NHWC RoIAlign forward on 3 x 13 x 17 maps, 7 x 7 bins, the edge + adaptive + random RoI family (every border rule occurs:
    asserted on A.stats), per element within roi_forward_bound (half storage: bracket, pinned share > 0.9); bins without samples are
    NaN and nothing else is; 64 guard rows stay intact.  The kernel named in the case is the one the launcher's rule selects for
    (dtype, C, sample_num, 16-byte alignment): f32 -> <float, 4> (C = 12: three channel lanes, which do not divide 256); half types,
    C / 8 dividing 256, sample_num 2 and aligned -> nhwc_bf16_s2 (C = 1024: two bin groups, 2048: one); the same but sample_num 0 or
    3, or a map that starts 8 bytes into its buffer (offset 4 elements: 16-byte unaligned, channels contiguous) -> generic <T, 8>;
    C = 24, 40 -> <T, 4>."""
    rois, A, nan = _family(sn)
    feat = _features(C, dtype, 17 * C + sn, offset)
    assert feat.data_ptr() % 16 == (2 * offset) % 16 and feat.is_contiguous()
    assert R.nhwc_kernel(C, dtype, sn, feat.data_ptr() % 16 == 0) == kernel
    got = _fwd_rows(feat, rois, R.PH, R.PW, sn, NHWC)
    ref, tol = T.roi_forward_bound(A, feat.reshape(-1, C))
    _check_rows('roi_align_fwd:' + kernel + ':C%d:s%d' % (C, sn), got, ref, tol, nan, dtype)
    assert float(ref[~nan].abs().max()) > 0.5


@pytest.mark.parametrize('sn', [2, 0])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: NAMES[d])
def test_roi_align_forward_nchw(dtype, sn):
    """roi_align_fwd_nchw<T> (layout NCHW always takes it), C = 8, same family and bound; ops.roi_align on the contiguous NCHW map
    returns the same bits, and on the channels_last map the NHWC kernel's."""
    rois, A, nan = _family(sn)
    feat = _features(8, dtype, 99 + sn)
    got = _fwd_rows(feat, rois, R.PH, R.PW, sn, NCHW)
    ref, tol = T.roi_forward_bound(A, feat.reshape(-1, 8))
    _check_rows('roi_align_fwd:nchw:s%d' % sn, got, ref, tol, nan, dtype)
    nchw = feat.permute(0, 3, 1, 2).contiguous()
    via_ops = ops.roi_align(nchw, rois, R.PH, R.SCALE, sn).permute(0, 2, 3, 1).reshape(-1, 8)
    assert torch.equal(torch.nan_to_num(via_ops.float(), nan=SENT), torch.nan_to_num(got.float(), nan=SENT))
    cl = ops.roi_align(nchw.contiguous(memory_format=torch.channels_last), rois, R.PH, R.SCALE, sn).permute(0, 2, 3, 1).reshape(-1, 8)
    _check_rows('ops.roi_align:channels_last:s%d' % sn, cl, ref, tol, nan, dtype)


def test_roi_align_forward_nchw_grid_stride():
    """K x C x 49 just above 65 536 x 256 at C = 8 (K = 42 800): the NCHW kernel's grid is capped and its grid-stride loop iterates.
    The RoIs are random draws (with repetition) from the family, so the reference is the family's, gathered per RoI in chunks; every
    element within roi_forward_bound."""
    K, C = 42800, 8
    assert (K - 1) * C * 49 <= 65536 * 256 < K * C * 49
    rois, A, _ = _family(2)
    idx = torch.randint(0, rois.shape[0], (K,), generator=torch.Generator().manual_seed(5)).to(DEV)
    feat = _features(C, torch.float32, 123)
    ref, tol = T.roi_forward_bound(A, feat.reshape(-1, C))
    ref, tol = ref.view(-1, 49, C), tol.view(-1, 49, C)
    got = _fwd_rows(feat, rois[idx].contiguous(), R.PH, R.PW, 2, NCHW).view(K, 49, C)
    worst, nbad = 0.0, 0
    for a in range(0, K, 8192):
        w, _, nb = R.ratio(got[a:a + 8192], R.Val(ref[idx[a:a + 8192]], tol[idx[a:a + 8192]]))
        worst, nbad = max(worst, w), nbad + nb
    print('RATIO roi_align_fwd:nchw:grid_stride f32 %.4g' % worst)
    assert worst <= 1.0, '%d elements over the bound, worst ratio %g' % (nbad, worst)


def test_roi_align_forward_split_half():
    """Split-half maps go through native.roi_align_fwd's cast path (f32 interpolation of the cast-back operand, the result stored as
    hi + lo): within roi_forward_bound on the cast-back operand plus the storage's 2^-22 relative + SPLIT_ABS (forward_kernel_refs)."""
    rois, A, nan = _family(2)
    C = 64
    stored = native.cast(_features(C, torch.float32, 31), native.SPLIT)
    operand = native.cast(stored, torch.float32)
    got = native.cast(native.roi_align_fwd(stored, rois, R.PH, R.PW, R.SCALE, 2, NHWC), torch.float32).reshape(-1, C)
    ref, tol = T.roi_forward_bound(A, operand.reshape(-1, C))
    _report('roi_align_fwd:cast_path', 'f16x2', got, R.Val(ref, tol + FK.SPLIT_REL * (ref.abs() + tol) + FK.SPLIT_ABS))


@pytest.mark.parametrize('dtype,C', [(torch.float32, 2048), (torch.float32, 6), (torch.bfloat16, 6), (torch.float16, 6)],
                         ids=lambda v: NAMES.get(v, str(v)) if isinstance(v, torch.dtype) else str(v))
def test_roi_align_forward_refusals(dtype, C):
    """NHWC maps no kernel takes (f32 with C / 4 > 256; C not divisible by 4) raise the library's error before any launch: the
    sentinel-filled output is untouched."""
    rois, _, _ = _family(2)
    assert R.nhwc_kernel(C, dtype, 2, True) is None
    feat = _features(C, dtype, 1)
    K = rois.shape[0]
    buf = torch.full((K * 49 * C,), SENT, dtype=dtype, device=DEV)
    with pytest.raises(native.HvrError):
        native.roi_align_fwd(feat, rois, R.PH, R.PW, R.SCALE, 2, NHWC, out=buf.view(K, R.PH, R.PW, C))
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


EXACT_CASES = [(NHWC, torch.float32, 12, 0, 'nhwc<float,4>'), (NHWC, torch.float32, 1024, 0, 'nhwc<float,4>')]
for _dt in (torch.bfloat16, torch.float16):
    EXACT_CASES += [(NHWC, _dt, 64, 0, 'nhwc_bf16_s2'), (NHWC, _dt, 2048, 0, 'nhwc_bf16_s2'), (NHWC, _dt, 64, 4, 'nhwc<T,8>'),
                    (NHWC, _dt, 24, 0, 'nhwc<T,4>')]
EXACT_CASES += [(NCHW, _dt, 8, 0, 'nchw') for _dt in (torch.float32, torch.bfloat16, torch.float16)]


@pytest.mark.parametrize('layout,dtype,C,offset,kernel', EXACT_CASES, ids=lambda v: NAMES.get(v, str(v)) if isinstance(v, torch.dtype) else str(v))
def test_roi_align_forward_exact_family(layout, dtype, C, offset, kernel):
    """The `<` / `<=` rules of the bilinear tap, bit for bit: RoI corners on multiples of 2 px, scale 1/16, 4 x 4 bins, 2 x 2 samples,
    integer features |f| <= 8 make every intermediate an f32 number (asserted by readout_refs), with samples exactly on -1, 0, interior
    integers, size - 1, size and just past it.  The device result equals the statement (f32) or the statement rounded once (bf16,
    f16), in every kernel: the case names the one the launcher's rule selects."""
    rois = R.roi_exact_rois()
    A, coords = R.roi_exact_matrix(rois)
    for axis in ('x', 'y'):
        assert min(R.roi_exact_landmarks(coords)[axis].values()) > 0
    n = R.EX_B * R.MAP_H * R.MAP_W * C
    flat = torch.zeros(n + offset, dtype=dtype, device=DEV)
    flat[offset:] = R.roi_exact_features(C).to(DEV).to(dtype).reshape(-1)
    feat = flat[offset:].view(R.EX_B, R.MAP_H, R.MAP_W, C)
    if layout == NHWC:
        assert R.nhwc_kernel(C, dtype, 2, feat.data_ptr() % 16 == 0) == kernel
    got = _fwd_rows(feat, rois.to(DEV), R.EX_PH, R.EX_PW, 2, layout)
    ref = R.roi_exact_statement(A.to(DEV), feat.reshape(-1, C))
    want = ref.float().to(dtype)
    bad = got != want
    print('RATIO roi_align_fwd:%s:exact %s %d' % (kernel, NAMES[dtype], int(bad.any())))
    assert not bool(bad.any()), '%d elements differ; first at flat index %d: got %r, statement %r' % (
        int(bad.sum()), int(bad.flatten().nonzero()[0]), float(got[bad][0]), float(ref[bad][0]))


# =============================================================================== hvr_det_decode
@pytest.mark.parametrize('img,sf', [((208, 272), 1.6), ((208, 272), 0.0), (None, 1.6), (None, 0.0)], ids=['clip_rescale', 'clip', 'rescale', 'plain'])
@pytest.mark.parametrize('Rr', [1, 63, 64, 65, 300])
def test_det_decode_against_f64(Rr, img, sf):
    """det_decode_kernel (one thread per row, 64-thread blocks: R on both sides of one block and several blocks) on a column slice of a
    wider tensor (ldl 160, cls_off 3, reg_off 40, 31 classes): boxes within the propagated delta2bbox bound, scores within the softmax
    bound and finite with row maxima of +-80.  dw / dh land below, inside and above the clamp (asserted at R >= 63); RoIs lie inside
    the image and across its border; with and without clipping, with rescaling (scale_factor 1.6) and without (0)."""
    wide, rois = R.det_case(Rr, 11 + Rr)
    cls, reg = wide[:, 3:34], wide[:, 40:44]
    if Rr >= 63:
        assert min(R.clamp_census(reg, R.DET_MEANS, R.DET_STDS)) > 0
    buf = torch.full((Rr + GUARD_ROWS, 160), SENT, device=DEV)
    buf[:Rr] = wide.to(DEV)
    scores, boxes = native.det_decode(buf[:Rr], 3, 40, 31, rois.to(DEV), R.DET_MEANS, R.DET_STDS, img, sf)
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(boxes).all())
    mode = 'f32'
    _report('det_decode:boxes:R%d' % Rr, mode, boxes, _dev(R.delta2bbox(rois[:, 1:], reg, R.DET_MEANS, R.DET_STDS, img, sf)))
    _report('det_decode:scores:R%d' % Rr, mode, scores, _dev(R.softmax(cls)))


# =============================================================================== hvr_rpn_proposals
@pytest.mark.parametrize('A,T_,nms_pre,exact', R.RPN_CASES)
def test_rpn_proposals_decode_against_f64(A, T_, nms_pre, exact):
    """native.rpn_proposals on inputs whose selection, order and suppression the f64 statement decides with room to spare (checked on
    the CPU for these very seeds), so every output row is attributable to an anchor: the row order is the statement's (each score is
    nearest to its own anchor's sigmoid among all anchors, which are >= 64 u apart), boxes and scores lie within the delta2bbox / sigmoid
    bounds, counts are exact, rows behind the count are zero.  The exact cases (dw = dh = 0, dyadic dx / dy, integer anchors) equal the
    statement bit for bit.  Regime, from hvr_rpn_proposals' rule: H W A <= nms_pre -> no selection; else T <= the wide-frames knob ->
    the chip-wide kernels, else one workgroup per frame.  A = 12 reads channel slices of one [T, H, W, 64] tensor (pitches 64 > A, 4 A)."""
    knob = native.rpn_wide_frames()
    assert 1 <= knob < 5
    n = R.RPN_H * R.RPN_W * A
    want_regime = 'unsorted' if nms_pre == 6000 else ('wide' if T_ == 1 else 'workgroup')
    assert R.rpn_regime(n, nms_pre, T_, R.RPN_NMS_POST, knob) == want_regime
    cls, reg = R.rpn_case(T_, A, R.RPN_SEEDS[(A, nms_pre, exact)], exact)
    base = R.rpn_base_anchors(A)
    if A == 12:
        fused = torch.full((T_, R.RPN_H, R.RPN_W, 64), SENT, device=DEV)
        fused[..., :A] = cls.view(T_, R.RPN_H, R.RPN_W, A).to(DEV)
        fused[..., A:5 * A] = reg.view(T_, R.RPN_H, R.RPN_W, 4 * A).to(DEV)
        dc, dr = fused[..., :A], fused[..., A:5 * A]
        assert dc.stride(2) == 64 and dr.stride(2) == 64
    else:
        dc, dr = cls.view(T_, R.RPN_H, R.RPN_W, A).to(DEV), reg.view(T_, R.RPN_H, R.RPN_W, 4 * A).to(DEV)
    props, counts = native.rpn_proposals(dc, dr, base, R.RPN_STRIDE, (0, 0, 0, 0), (1, 1, 1, 1), R.RPN_IMG, nms_pre, R.RPN_NMS_POST,
                                         R.RPN_MAX_NUM, R.RPN_NMS_THR)
    props, counts = props.cpu(), counts.cpu()
    tag = 'rpn_proposals:%s:A%d' % (want_regime, A) + (':exact' if exact else '')
    for t in range(T_):
        st = R.rpn_statement(cls[t], reg[t], base, nms_pre, R.RPN_NMS_POST, R.RPN_MAX_NUM)
        m = st['order'].numel()
        assert int(counts[t]) == m, (t, int(counts[t]), m)
        assert bool((props[t, m:] == 0).all())
        all_scores = R.sigmoid(cls[t]).v
        nearest = (props[t, :m, 4].double()[:, None] - all_scores[None, :]).abs().argmin(1)
        assert torch.equal(nearest, st['order']), 'frame %d: rows are not the statement\'s anchors in its order' % t
        if exact:
            assert torch.equal(props[t, :m, :4], st['boxes'].v.float())
        _report(tag + ':boxes', 'f32', props[t, :m, :4], st['boxes'])
        _report(tag + ':scores', 'f32', props[t, :m, 4], st['scores'])


# =============================================================================== hvr_box_targets
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)


@pytest.mark.parametrize('scatter', [False, True])
@pytest.mark.parametrize('k', [1, 7, 256])
def test_box_targets_against_f64(k, scatter):
    """box_targets_kernel, n = 300 proposals, 250 sampled indices: the encoded deltas within the bbox2delta bound (logf at 3 ulp,
    correctly rounded divisions; targets.hip is built without contraction), labels / weights exact, for pos_weight -1 and 2, gt_labels
    given and None, counts with zero positives and with zero negatives; rows beyond counts[0] + counts[1] (and, scattered, rows
    no index names) stay zero.  Then the pair box_targets -> det_decode returns the ground truth within the two bounds added."""
    n, num = 300, 250
    boxes, gts, gt_labels, gt_inds, inds = R.targets_case(n, k, 40 + k)
    inds = inds[:num].contiguous()
    d = lambda t: None if t is None else t.to(DEV)
    for counts in ((100, 120), (0, 200), (250, 0)):
        for pos_weight, labels_in in ((-1.0, gt_labels), (2.0, None)):
            cnt = torch.tensor(counts, dtype=torch.int32)
            got = native.box_targets(d(boxes), d(gts), d(labels_in), d(gt_inds), d(inds), d(cnt), MEANS, STDS, pos_weight, scatter)
            labels, lw, bt, bw = R.box_targets(boxes, gts, labels_in, gt_inds, inds, cnt, MEANS, STDS, pos_weight, scatter)
            assert torch.equal(got[0].cpu(), labels) and torch.equal(got[1].cpu().double(), lw) and torch.equal(got[3].cpu().double(), bw)
            _report('box_targets:k%d:%s:np%d' % (k, 'scatter' if scatter else 'rows', counts[0]), 'f32', got[2].cpu(), bt)
            untouched = bw[:, 0] == 0
            assert bool(untouched.any()) == (scatter or sum(counts) < num) and bool((got[2].cpu()[untouched] == 0).all())
    # round trip on the last call's positives (all 250 sampled rows): decode the device's targets with the device's decoder
    rows = inds if scatter else torch.arange(num)
    t_dev = got[2][d(rows)]
    p, g = boxes[inds], gts[gt_inds[inds] - 1]
    wide = torch.zeros((num, 8), device=DEV)
    wide[:, 4:] = t_dev
    _, back = native.det_decode(wide, 0, 4, 2, torch.cat([torch.zeros(num, 1), p], 1).to(DEV), MEANS, STDS, None, 0.0)
    bound = R.delta2bbox(p, R.bbox2delta(p, g, MEANS, STDS), MEANS, STDS)
    _report('box_targets->det_decode:k%d' % k, 'f32', back.cpu(), R.Val(g.double(), bound.e + (bound.v - g.double()).abs()))


# =============================================================================== hvr_max_iou_assign
@pytest.mark.parametrize('n,k,seed,pos,neg,min_pos', R.ASSIGN_CASES)
def test_max_iou_assign_against_f64(n, k, seed, pos, neg, min_pos):
    """assign_max_kernel / assign_final_kernel (256-thread blocks: n on both sides of one block, several blocks; k = 1 and the
    256-gt limit) on boxes that are columns 1..4 of an RoI tensor (row pitch 5) with some rows masked by `valid`: max_overlaps within
    the IoU bound (-1 exactly on masked rows), gt_inds equal to the f64 assignment -- every threshold comparison holds by more than
    the IoU bound on these inputs (checked on the CPU for these seeds), and the "equals the gt's maximum" rule is exercised by a box
    duplicated bit for bit."""
    rois5, gts, valid = R.assign_case(n, k, seed)
    inds, mo, margin = R.max_iou_assign(rois5[:, 1:], gts, pos, neg, min_pos, valid)
    assert margin > 0
    dev = rois5.to(DEV)
    view = dev[:, 1:]
    assert view.stride(0) == 5 and view.stride(1) == 1
    got_inds, got_mo = native.max_iou_assign(view, gts.to(DEV), pos, neg, min_pos, valid.to(DEV))
    _report('max_iou_assign:n%d:k%d' % (n, k), 'f32', got_mo.cpu(), mo)
    bad = got_inds.cpu() != inds
    assert not bool(bad.any()), '%d rows assigned differently; first row %d: got %d, statement %d' % (
        int(bad.sum()), int(bad.nonzero()[0]), int(got_inds.cpu()[bad][0]), int(inds[bad][0]))
    if n > 2:
        assert int(got_inds[0]) == int(got_inds[n - 1]) > 0
