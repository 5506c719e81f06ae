"""The f64 statements of tests/readout_refs.py, on the CPU: each against the committed reference recordings it overlaps (g2, g4,
g8, g12) and against the f32 oracle at the same shapes, within the bounds the GPU tests use; the conditions on the GPU tests' inputs
(branches reached, landmarks hit, decision margins positive); and for each statement plausible mistakes, which must move the result
by at least ten times the largest bound the GPU test allows on the same inputs."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import readout_refs as R
from tests import train_kernel_refs as T
from tests.golden import cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def O():
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def _within(got, val, what):
    worst, at, nbad = R.ratio(torch.as_tensor(np.asarray(got)), val)
    assert worst <= 1.0, '%s: %d elements over the bound, worst ratio %g at flat index %d' % (what, nbad, worst, at)
    return worst


def _moves(wrong, right, factor=10.0):
    """the mistake moves at least one element by >= factor x the LARGEST bound on these inputs"""
    return float((wrong.v - right.v).abs().max()) >= factor * float(right.e.max())


# ------------------------------------------------------------------------------- the Val machinery
def test_val_bounds_cover_f32_evaluations():
    """An f32 evaluation by torch of sums, products, quotients, exp and log lies within Val's bound of the f64 value, and the bound
    is not slack by more than a small factor (a vacuous bound would pass every kernel)."""
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.randn(4096, generator=g) * 5 for _ in range(3))
    got = ((a * b + c) / (b.abs() + 1.0)).exp().log()
    va, vb, vc = R.Val(a), R.Val(b), R.Val(c)
    val = ((va * vb + vc) / (R.Val(b.abs()) + 1.0)).exp().log()
    worst, _, nbad = R.ratio(got, val)
    assert nbad == 0 and 0.01 < worst <= 1.0, worst
    assert float((val.e / val.v.abs().clamp(min=1.0)).max()) < 200 * R.U
    assert float(R.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.75], dtype=torch.float64)).sub(torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24])).abs().max()) == 0


# ------------------------------------------------------------------------------- RoIAlign
def test_roi_statement_matches_g4_and_oracle(O):
    """g4 (recorded from the f32 restatement, which the oracle reproduces bit for bit) within roi_forward_bound of A F; NaN exactly on
    the bins without samples."""
    g = gold('g4_roi_align')
    for name, scale, out in (('m15', 1 / 16, 7), ('m38', 1 / 16, 7), ('gc', 1 / 8, 3)):
        feat, rois = torch.from_numpy(g[name + '_feat']), torch.from_numpy(g[name + '_rois'])
        B, Cc, H, W = feat.shape
        F = feat.permute(0, 2, 3, 1).reshape(-1, Cc)
        for sn in (2, 0):
            A = T.roi_align_matrix(rois, B, H, W, out, out, scale, sn)
            ref, tol = T.roi_forward_bound(A, F)
            nan = R.nan_rows(A, out * out)
            for src in (torch.from_numpy(g['%s_out_s%d' % (name, sn)]), O.roi_align(feat, rois, out, scale, sn)):
                got = src.permute(0, 2, 3, 1).reshape(-1, Cc)
                assert torch.equal(torch.isnan(got).any(1), nan) and torch.equal(torch.isnan(got).all(1), nan)
                assert bool(((got.double() - ref).abs() <= tol)[~nan].all()), (name, sn)
            assert sn == 2 or name == 'gc' or bool(nan.any())


def test_roi_family_reaches_every_border_rule_and_mistakes_show():
    """The RoIs of the GPU forward tests on the 3 x 13 x 17 maps: every border rule of the bilinear tap occurs, adaptive sampling has
    bins without samples, and three mistakes (sample offset without the half, the window (-1, size - 1], the mean over the live
    samples only) each move the result by >= 10 x the largest bound."""
    rois = R.roi_family()
    g = torch.Generator().manual_seed(3)
    F = torch.randn((R.MAP_B * R.MAP_H * R.MAP_W, 8), generator=g)
    for sn in (2, 0, 3):
        A = T.roi_align_matrix(rois, R.MAP_B, R.MAP_H, R.MAP_W, R.PH, R.PW, R.SCALE, sn)
        for k in ('y_neg', 'x_neg', 'y_clamped', 'x_clamped', 'y_dead_only', 'x_dead_only', 'live'):
            assert A.stats[k] > 0, (sn, k, A.stats)
        assert bool(R.nan_rows(A).any()) == (sn == 0)
        ref, tol = T.roi_forward_bound(A, F)
        big = 10 * float(tol.max())
        for kw in (dict(off_frac=0.0), dict(border_mut=True)):
            wrong = T.apply(T.roi_align_matrix(rois, R.MAP_B, R.MAP_H, R.MAP_W, R.PH, R.PW, R.SCALE, sn, **kw), F)
            assert float((wrong - ref).abs().max()) >= big, kw
        frac = R.live_fraction(A)
        part = (frac > 0) & (frac < 1)
        assert bool(part.any())
        by_live = ref / frac.clamp(min=1e-9)
        assert float((by_live - ref)[part[:, 0]].abs().max()) >= big


def test_roi_exact_family_is_exact_and_hits_the_landmarks(O):
    """Every intermediate equals its f32 round trip (asserted inside roi_exact_matrix / roi_exact_statement); samples sit exactly on
    -1, 0, interior integers, size - 1, size and just past it on both axes; the statement agrees with the general matrix; the f32
    oracle reproduces it bit for bit; the border mistakes (window (-1, size - 1], and y <= -1 dead) each change an element."""
    rois = R.roi_exact_rois()
    assert bool((rois[:, 1:3] % 2 == 0).all()) and bool(((rois[:, 3:] + 1) % 2 == 0).all())
    A, coords = R.roi_exact_matrix(rois)
    marks = R.roi_exact_landmarks(coords)
    for axis in ('x', 'y'):
        for k, n in marks[axis].items():
            assert n > 0, (axis, k, marks)
    feat = R.roi_exact_features(8)
    F = feat.reshape(-1, 8)
    ref = R.roi_exact_statement(A, F)
    assert float(ref.abs().max()) > 1
    general = T.apply(T.roi_align_matrix(rois, R.EX_B, R.MAP_H, R.MAP_W, R.EX_PH, R.EX_PW, R.SCALE, 2), F)
    assert torch.equal(general, ref)
    got = O.roi_align(feat.permute(0, 3, 1, 2).contiguous(), rois, R.EX_PH, R.SCALE, 2).permute(0, 2, 3, 1).reshape(-1, 8)
    assert torch.equal(got.double(), ref)
    for mistake in ('border_mut', 'neg_le'):
        wrong = R.roi_exact_statement(R.roi_exact_matrix(rois, mistake)[0], F)
        assert int((wrong != ref).sum()) >= 1, mistake


def test_kernel_selection_rule():
    """readout_refs.nhwc_kernel restates the launcher's documented rule: the kernels the GPU cases name, and the three refusals."""
    bf = torch.bfloat16
    assert [R.nhwc_kernel(c, torch.float32, 2, True) for c in (8, 12, 64, 1024, 2048, 6)] == ['nhwc<float,4>'] * 4 + [None, None]
    assert [R.nhwc_kernel(c, bf, 2, True) for c in (8, 64, 1024, 2048)] == ['nhwc_bf16_s2'] * 4
    assert R.nhwc_kernel(64, bf, 0, True) == R.nhwc_kernel(64, bf, 3, True) == R.nhwc_kernel(64, bf, 2, False) == 'nhwc<T,8>'
    assert R.nhwc_kernel(24, bf, 2, True) == R.nhwc_kernel(40, bf, 2, True) == 'nhwc<T,4>' and R.nhwc_kernel(6, bf, 2, True) is None


# ------------------------------------------------------------------------------- decode
def test_delta2bbox_matches_g2_g8_and_oracle(O):
    """g2 (delta2bbox of the reference: RPN stds, RCNN stds, no clip) and g8 (RCNN read-out: boxes and softmax scores), and the f32
    oracle on the GPU test's own inputs, within the propagated bound."""
    g = gold('g2_delta2bbox')
    rois, deltas = C.delta2bbox_case()
    z, rc = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    _within(g['out_rpn'], R.delta2bbox(rois, deltas, z, (1., 1., 1., 1.), (600, 1000)), 'g2 rpn')
    _within(g['out_rcnn'], R.delta2bbox(rois, deltas, z, rc, (600, 1000)), 'g2 rcnn')
    _within(g['out_noclip'], R.delta2bbox(rois, deltas, z, rc, None), 'g2 noclip')
    g8 = gold('g8_det')
    rois5, cls, reg = C.det_case()
    _within(g8['bboxes'], R.delta2bbox(rois5[:, 1:], reg, z, rc, (600, 1000)), 'g8 boxes')
    _within(g8['scores'], R.softmax(cls), 'g8 scores')
    for Rr in (1, 65, 300):
        wide, rois5 = R.det_case(Rr, 11 + Rr)
        cls, reg = wide[:, 3:34], wide[:, 40:44]
        for img, sf in (((208, 272), 1.6), (None, 0.0)):
            val = R.delta2bbox(rois5[:, 1:], reg, R.DET_MEANS, R.DET_STDS, img, sf)
            bb, sc = O.get_det_bboxes(rois5, cls.contiguous(), reg.contiguous(), img, np.float32(sf) if sf > 0 else 1.0, sf > 0, None)
            _within(bb, val, 'oracle boxes')
            _within(sc, R.softmax(cls), 'oracle scores')


def test_decode_inputs_and_mistakes():
    """The det_decode inputs put dw / dh below, inside and above the clamp, RoIs inside and across the border, row maxima at +-80 with
    finite scores; and the four decode mistakes each move a box by >= 10 x the largest bound."""
    wide, rois5 = R.det_case(300, 311)
    cls, reg = wide[:, 3:34], wide[:, 40:44]
    below, inside, above = R.clamp_census(reg, R.DET_MEANS, R.DET_STDS)
    assert min(below, inside, above) > 20
    assert set(cls.max(1).values.tolist()) == {80.0, -80.0}
    sm = R.softmax(cls)
    assert bool(torch.isfinite(sm.v).all()) and float((sm.v.sum(1) - 1).abs().max()) < 1e-12 and float((sm.e / sm.v).max()) < 200 * R.U
    b = rois5[:, 1:]
    assert int(((b[:, 0] < 0) | (b[:, 2] > 271)).sum()) > 10 and int(((b[:, 0] > 0) & (b[:, 2] < 271) & (b[:, 1] > 0) & (b[:, 3] < 207)).sum()) > 10
    for img, sf, mistakes in (((208, 272), 1.6, ('no_plus1', 'clamp_after_exp', 'clip_to_img', 'mul_scale')), (None, 0.0, ('no_plus1', 'clamp_after_exp'))):
        right = R.delta2bbox(b, reg, R.DET_MEANS, R.DET_STDS, img, sf)
        for m in mistakes:
            assert _moves(R.delta2bbox(b, reg, R.DET_MEANS, R.DET_STDS, img, sf, mistake=m), right), m


@pytest.mark.parametrize('A,T_,nms_pre,exact', R.RPN_CASES)
def test_rpn_inputs_are_decided_with_room(A, T_, nms_pre, exact):
    """For every call of the GPU test: neighbouring sigmoids at least 64 u apart beyond their bounds (asserted in rpn_statement), every
    pair of decoded boxes further from the NMS threshold than the IoU bound the box bounds imply, no two decoded boxes identical, and
    both outcomes of the NMS occur.  The exact family's boxes carry no error beyond the clip (dyadic shifts of integer anchors)."""
    cls, reg = R.rpn_case(T_, A, R.RPN_SEEDS[(A, nms_pre, exact)], exact)
    base = R.rpn_base_anchors(A)
    for t in range(T_):
        st = R.rpn_statement(cls[t], reg[t], base, nms_pre, R.RPN_NMS_POST, R.RPN_MAX_NUM)
        assert st['nms_margin'] > 0 and st['distinct'], (t, st['nms_margin'], st['distinct'])
        n_in = min(nms_pre, cls[t].numel())
        assert 0 < st['order'].numel() <= min(n_in, R.RPN_MAX_NUM)
        assert exact or st['order'].numel() < n_in                     # something was suppressed (or cut)
        if exact:
            assert torch.equal(st['boxes'].v, st['boxes'].v.float().double())
    if not exact:
        mr = R.max_ratio_of()
        assert int((reg[:, :, 2:] > mr).sum()) > 0 and int((reg[:, :, 2:] < -mr).sum()) > 0


def test_rpn_statement_matches_oracle(O):
    """The f32 oracle's RPN read-out (selection, decode, NMS, cut) returns the statement's rows in the statement's order, boxes and
    scores within the bounds."""
    for A, T_, nms_pre, exact in R.RPN_CASES[:4] + R.RPN_CASES[-3:]:
        cls, reg = R.rpn_case(T_, A, R.RPN_SEEDS[(A, nms_pre, exact)], exact)
        base = R.rpn_base_anchors(A)
        st = R.rpn_statement(cls[0], reg[0], base, nms_pre, R.RPN_NMS_POST, R.RPN_MAX_NUM)
        cfg = dict(nms_pre=nms_pre, nms_post=R.RPN_NMS_POST, max_num=R.RPN_MAX_NUM, nms_thr=R.RPN_NMS_THR, min_bbox_size=0)
        c = cls[0].view(R.RPN_H, R.RPN_W, A).permute(2, 0, 1).contiguous()
        r = reg[0].view(R.RPN_H, R.RPN_W, 4 * A).permute(2, 0, 1).contiguous()
        out = O.rpn_get_bboxes_single(c, r, R.rpn_anchors(base), R.RPN_IMG + (3,), cfg)
        assert out.shape[0] == st['order'].numel()
        _within(out[:, :4], st['boxes'], 'oracle rpn boxes')
        _within(out[:, 4], st['scores'], 'oracle rpn scores')


# ------------------------------------------------------------------------------- encode and IoU
def test_bbox2delta_and_iou_match_g12_and_oracle(O):
    """g12: the reference's RCNN bbox targets of the sampled positives and the RPN assigner's max overlaps / gt indices; and the f32
    oracle on the GPU test's inputs."""
    g = gold('g12_targets')
    tc = C.target_case()
    gt_b = tc['gt_bboxes']
    k = gt_b.shape[0]
    pos = torch.from_numpy(g['rcnn_pos_inds']).long()
    gt_of = torch.where(pos < k, pos + 1, torch.from_numpy(g['rcnn_gt_inds']).long()[(pos - k).clamp(min=0)])
    rois = torch.from_numpy(g['rcnn_rois'])[:pos.numel()]
    val = R.bbox2delta(rois, gt_b[gt_of - 1], (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2))
    _within(g['rcnn_bbox_targets'][:pos.numel()], val, 'g12 rcnn targets')
    anchors = O.grid_anchors(O.gen_base_anchors(16, [4, 8, 16, 32], [0.5, 1.0, 2.0]), (38, 63), 16)[torch.from_numpy(g['inside']).bool()]
    a = C.RPN_TRAIN_CFG['assigner']
    inds, mo, _ = R.max_iou_assign(anchors, gt_b, a['pos_iou_thr'], a['neg_iou_thr'], a['min_pos_iou'])
    _within(g['rpn_max_overlaps'], mo, 'g12 max overlaps')
    assert torch.equal(inds, torch.from_numpy(g['rpn_gt_inds']).long())
    boxes, gts, _, gt_inds, _ = R.targets_case(300, 7, 3)
    _within(O.bbox2delta(boxes, gts[gt_inds - 1], (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)),
            R.bbox2delta(boxes, gts[gt_inds - 1], (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)), 'oracle bbox2delta')
    rois5, gts, valid = R.assign_case(257, 256, 7 * 257 + 256)
    _within(O.bbox_overlaps(rois5[:, 1:].contiguous(), gts), R.iou(R.Val(rois5[:, 1:]), R.Val(gts)), 'oracle iou')


def test_encode_mistakes_and_round_trip():
    """log(pw / gw), no stds, and an IoU without the +1 each move the result by >= 10 x the largest bound; decoding the encoded
    deltas returns the ground truth within the two bounds added."""
    means, stds = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    boxes, gts, _, gt_inds, _ = R.targets_case(300, 7, 3)
    g = gts[gt_inds - 1]
    right = R.bbox2delta(boxes, g, means, stds)
    for m in ('inverted_log', 'no_stds'):
        assert _moves(R.bbox2delta(boxes, g, means, stds, mistake=m), right), m
    back = R.delta2bbox(boxes, right, means, stds)            # the decode's bound with the encode's carried through it
    assert bool(((back.v - g.double()).abs() <= back.e).all()) and float((back.e / g.abs().clamp(min=1.0)).max()) < 1e-4
    rois5, gts2, _ = R.assign_case(257, 256, 7 * 257 + 256)
    ov = R.iou(R.Val(rois5[:, 1:]), R.Val(gts2))
    assert _moves(R.iou(R.Val(rois5[:, 1:]), R.Val(gts2), mistake='no_plus1'), ov)


@pytest.mark.parametrize('n,k,seed,pos,neg,min_pos', R.ASSIGN_CASES)
def test_assign_inputs_are_decided_with_room(n, k, seed, pos, neg, min_pos):
    """Every comparison the assignment depends on holds by more than the IoU bound (margin > 0), positives, background, ignored and
    masked rows all occur (n > 2), and the bit-for-bit duplicate is assigned like its twin through the "equals the gt's maximum" rule."""
    rois5, gts, valid = R.assign_case(n, k, seed)
    inds, mo, margin = R.max_iou_assign(rois5[:, 1:], gts, pos, neg, min_pos, valid)
    assert margin > 0, margin
    if n > 2:
        assert inds[0] == inds[n - 1] and inds[0] > 0 and (k > 1 or inds[0] == 1)
        assert int((inds > 0).sum()) > 2 and int((inds == 0).sum()) > 0 and int((~valid).sum()) > 0 and bool((inds[~valid] == -1).all())
        assert k == 1 or int(((inds == -1) & valid).sum()) > 0
