"""Pins the CPU oracle (oracle/) to the reference: golden vectors produced by the reference's own
modules (tests/golden/make_golden.py), the reference's doctest known-answers, the reference's
nms_cpu.cpp compiled unmodified (oracle/_ref, when present; its keep lists recorded), and hand-derived RoIAlign geometry.
Runs on CPU (-m "not gpu")."""
import os
import subprocess

import numpy as np
import pytest
import torch

from hvrnet_amd import synthetic as S
from tests.golden import cases as C, numerics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module', autouse=True)
def recorded_thread_count():
    """How a product or a reduction is split over threads moves its float32 sum: replay on the thread count the vectors were
    recorded with (tests/golden/numerics.py)."""
    n = torch.get_num_threads()
    torch.set_num_threads(numerics.THREADS)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope='module')
def O():
    if not os.path.exists(os.path.join(ROOT, 'oracle', 'libhvr_oracle.so')):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'oracle')], check=True)
    from oracle import hvr_oracle
    return hvr_oracle


def gold(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def close(a, b, rtol=1e-5, atol=1e-5):
    torch.testing.assert_close(torch.as_tensor(np.asarray(a)).float(), torch.as_tensor(np.asarray(b)).float(), rtol=rtol, atol=atol)


def test_g1_anchors(O):
    g = gold('g1_anchors')
    base = O.gen_base_anchors(16, [4, 8, 16, 32], [0.5, 1.0, 2.0])
    assert np.array_equal(base.numpy(), g['base'])
    assert base[0].tolist() == [-37., -15., 52., 30.]
    grid = O.grid_anchors(base, (38, 63), 16)
    assert grid.shape[0] == int(g['grid_count']) == 28728
    assert np.array_equal(grid[:24].numpy(), g['grid_first']) and np.array_equal(grid[-24:].numpy(), g['grid_last'])
    assert np.array_equal(grid.double().sum(0).numpy(), g['grid_sum'])
    # doctest mmdet/core/anchor/anchor_generator.py:6-14
    doc = O.grid_anchors(O.gen_base_anchors(9, [1.], [1.]), (2, 2), 16)
    assert doc.tolist() == [[0., 0., 8., 8.], [16., 0., 24., 8.], [0., 16., 8., 24.], [16., 16., 24., 24.]]
    assert np.array_equal(doc.numpy(), g['doctest'])


def test_g2_delta2bbox(O):
    g = gold('g2_delta2bbox')
    rois, deltas = C.delta2bbox_case()
    assert np.array_equal(rois.numpy(), g['rois'])
    close(O.delta2bbox(rois, deltas, [0., 0., 0., 0.], [1., 1., 1., 1.], (600, 1000)), g['out_rpn'], 0, 0)
    close(O.delta2bbox(rois, deltas, [0., 0., 0., 0.], [0.1, 0.1, 0.2, 0.2], (600, 1000)), g['out_rcnn'], 0, 0)
    close(O.delta2bbox(rois, deltas, [0., 0., 0., 0.], [0.1, 0.1, 0.2, 0.2], None), g['out_noclip'], 0, 0)
    # doctest mmdet/core/bbox/transforms.py:63-76
    out = O.delta2bbox(torch.as_tensor(g['doc_rois']), torch.as_tensor(g['doc_deltas']), max_shape=(32, 32))
    close(out, [[0.0000, 0.0000, 1.0000, 1.0000], [0.2817, 0.2817, 4.7183, 4.7183], [0.0000, 0.6321, 7.3891, 0.3679],
                [5.8967, 2.9251, 5.5033, 3.2749]], 0, 5e-5)
    close(out, g['doc_out'], 0, 0)


def test_g3_nms_against_reference_cpu_kernel(O):
    g = gold('g3_nms')
    for name, dets, thr in C.nms_cases():
        _, keep = O.nms(dets, thr)
        assert keep.tolist() == g[name + '_keep'].tolist(), name
    # doctest mmdet/ops/nms/nms_wrapper.py:26-36 (3 survive), reference answer [0, 3, 4]
    assert g['doc_keep'].tolist() == [0, 3, 4]
    # `>=`: IoU exactly 0.5 at thr 0.5 suppresses (nms_cpu.cpp:55)
    assert g['tie_iou_half_keep'].tolist() == [0, 3]
    d, k = O.nms(torch.zeros((0, 5)), 0.5)
    assert d.shape == (0, 5) and k.numel() == 0


def test_nms_against_live_reference_build(O):
    """Random boxes against nms_cpu.cpp's keep lists as recorded (g17), and against the live build too where this checkout has one."""
    from oracle import build_ref
    g = gold('g17_nms_random')
    ref = build_ref.load_ref()
    for seed in range(5):
        dets = C.boxes(500, 4000 + seed)
        keep = O.nms(dets, 0.5)[1].tolist()
        assert keep == g['seed%d_keep' % seed].tolist(), seed
        if ref is not None:
            assert keep == ref.nms(dets, 0.5).tolist(), seed


def test_roi_align_hand_derived_geometry(O):
    """The reference RoIAlign is CUDA-only, so the restatement is pinned by closed-form cases.
    On a feature f(y, x) = a*y + b*x + c bilinear interpolation is exact, so each output bin equals
    f at the mean of its sample points (roi_align_kernel.cu:78-116 geometry, '+1' end coordinate)."""
    H, W = 15, 20
    a, b, c = 0.5, -0.25, 2.0
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    feat = (a * ys + b * xs + c)[None, None].repeat(1, 2, 1, 1)
    feat[:, 1] *= 2
    rois = torch.tensor([[0, 16., 32., 111., 95.], [0, 40., 40., 40., 40.]])  # second: 1x1 pixel box -> width (0+1)*s
    out = O.roi_align(feat, rois, 7, 1 / 16, 2)
    for k in range(2):
        x1, y1, x2, y2 = rois[k, 1:].tolist()
        sw, sh = x1 / 16, y1 / 16
        bw, bh = ((x2 + 1) / 16 - sw) / 7, ((y2 + 1) / 16 - sh) / 7
        for ph in range(7):
            for pw in range(7):
                cy, cx = sh + (ph + 0.5) * bh, sw + (pw + 0.5) * bw  # mean of the 2x2 sample grid
                want = a * cy + b * cx + c
                assert abs(out[k, 0, ph, pw].item() - want) < 1e-4
                assert abs(out[k, 1, ph, pw].item() - 2 * want) < 2e-4
    # constant map, box partly outside: samples beyond (-1, H)x(-1, W) contribute 0 but still count
    ones = torch.ones((1, 1, 4, 4))
    o = O.roi_align(ones, torch.tensor([[0, -64., -64., 31., 31.]]), 2, 1 / 16, 2)
    # box spans [-4, 2) in feature coords, bins of 3: first bin samples at -3.25, -1.75 -> both < -1 -> 0
    assert torch.allclose(o[0, 0], torch.tensor([[0., 0.], [0., 1.]]))
    # malformed roi (x2 < x1 - 1): width clamps to 0, every sample sits on the start point
    o = O.roi_align(feat, torch.tensor([[0, 64., 48., 10., 10.]]), 3, 1 / 16, 2)
    assert torch.allclose(o[0, 0], torch.full((3, 3), a * 3.0 + b * 4.0 + c))
    # backward is the adjoint of forward: <fwd(f), g> == <f, bwd(g)>
    g = torch.Generator().manual_seed(5)
    f = torch.randn((2, 3, 9, 11), generator=g)
    r = torch.tensor([[0, 3., 5., 100., 90.], [1, 40., 10., 150., 120.], [1, -20., -20., 60., 50.]])
    go = torch.randn((3, 3, 4, 4), generator=g)
    lhs = (O.roi_align(f, r, 4, 1 / 16, 2) * go).double().sum()
    rhs = (f * O.roi_align_backward(go, r, f.shape, 1 / 16, 2)).double().sum()
    assert abs(lhs - rhs) < 1e-3 * max(1.0, abs(lhs))


def test_roi_align_restatement_reproduces_g4(O):
    """G4 pins the C restatement of ROIAlignForward against drift (the expected outputs were produced by it, the fixture says
    so: the reference's kernel has no CPU path, roi_align.py:27-28).  Bit for bit; NaN where the reference's arithmetic gives
    0 / 0 (adaptive sample count of a zero-size box)."""
    g = gold('g4_roi_align')
    assert str(g['roi_align_source']) == 'oracle'
    for name, scale, out in (('m15', 1 / 16, 7), ('m38', 1 / 16, 7), ('gc', 1 / 8, 3)):
        feat, rois = torch.from_numpy(g[name + '_feat']), torch.from_numpy(g[name + '_rois'])
        for sn in (2, 0):
            got = O.roi_align(feat, rois, out, scale, sn).numpy()
            assert np.array_equal(got, g['%s_out_s%d' % (name, sn)], equal_nan=True)
    # the special boxes of the fixture behave as roi_align_kernel.cu:16-45,78-116 says they must
    feat, rois = torch.from_numpy(g['m15_feat']), torch.from_numpy(g['m15_rois'])
    o2 = g['m15_out_s2']
    assert np.all(o2[5] == 0)                                         # fully outside: every sample out of bounds -> 0
    b = int(rois[6, 0])
    assert np.allclose(o2[6], feat[b, :, 0, 0].numpy()[:, None, None])  # samples in (-1, 0) clamp to pixel (0, 0)
    assert np.isnan(g['m15_out_s0'][2]).all()                         # malformed box, adaptive sampling: 0 samples -> 0 / 0


def test_roi_align_against_an_independent_interpolator(O):
    """Second pin for the CUDA-only RoIAlign: on RANDOM (non-linear) features the restatement must equal the average of
    torch.nn.functional.grid_sample's bilinear values (align_corners=True, an interpolator this build did not write) at the
    2 x 2 sample points of every bin (roi_align_kernel.cu:78-116: start + (p + (i + .5) / 2) * bin, end = (x2 + 1) * scale).
    Interior boxes exercise the plain 4-tap rule; boxes that stick out exercise its border rule (:29-53): a point in
    [-1, 0) or (H - 1, H] is clamped onto the edge pixel -- grid_sample's padding_mode='border' -- and a point beyond
    [-1, H] x [-1, W] contributes 0 but still counts in the mean."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 5, 19, 27
    feat = torch.randn((B, C, H, W), generator=g)
    rois = torch.tensor([[0, 33., 21., 250., 170.], [1, 100.5, 40.25, 180.75, 260.5], [0, 5., 7., 60., 44.],
                         [1, -30., -20., 120., 90.], [0, 300., 200., 470., 330.], [1, -300., 10., -100., 80.]])
    ph = pw = 7
    got = O.roi_align(feat, rois, ph, 1 / 16, 2)
    for k in range(rois.shape[0]):
        b, x1, y1, x2, y2 = rois[k].tolist()
        sw, sh = x1 / 16, y1 / 16
        bw, bh = max((x2 + 1) / 16 - sw, 0.) / pw, max((y2 + 1) / 16 - sh, 0.) / ph
        ys = torch.tensor([sh + p * bh + (i + .5) * bh / 2 for p in range(ph) for i in range(2)])       # [14]
        xs = torch.tensor([sw + p * bw + (i + .5) * bw / 2 for p in range(pw) for i in range(2)])
        yy, xx = torch.meshgrid(ys, xs, indexing='ij')
        inside = ((yy >= -1) & (yy <= H) & (xx >= -1) & (xx <= W)).float()
        grid = torch.stack([xx / (W - 1) * 2 - 1, yy / (H - 1) * 2 - 1], dim=-1)[None]                    # x first, in [-1, 1]
        vals = F.grid_sample(feat[int(b)][None], grid.float(), mode='bilinear', padding_mode='border', align_corners=True)[0]
        want = (vals * inside).view(C, ph, 2, pw, 2).mean(dim=(2, 4))
        close(got[k], want, 1e-5, 1e-5)
    assert got[5].abs().max() == 0                                              # entirely left of x = -1


def test_g5_relation_stage(O):
    g = gold('g5_relation')
    sd_s, sd_h = S.synth_state_dict('selsa'), S.synth_state_dict('hvr')
    x = C.relation_input()
    cur = dict(start=32, length=32)
    close(O.relation_stage(x, sd_s, 'bbox_head', 1, 96), g['y_all'], 1e-4, 1e-5)
    close(O.relation_stage(x, sd_h, 'bbox_head', 4, 96, cur_range=cur, output_cur_only=True), g['y_key'], 1e-4, 1e-5)
    close(O.relation_stage(x, sd_s, 'bbox_head', 2, 64), g['y_trunc'], 1e-4, 1e-5)


def test_g6_g7_heads(O):
    feats = C.roi_feat_input()
    cur = dict(start=32, length=32)
    g6, g7 = gold('g6_selsa_head'), gold('g7_hvr_head')
    cls, reg = O.selsa_head_forward(feats, S.synth_state_dict('selsa'), cur, 32, 3)
    close(cls, g6['cls'], 1e-4, 1e-4)
    close(reg, g6['reg'], 1e-4, 1e-4)
    cls_l, reg_l = O.hvr_head_forward_test(feats, S.synth_state_dict('hvr'), cur, 32, 3)
    close(cls_l[0], g7['cls_branch'], 1e-4, 1e-4)
    close(cls_l[1], g7['cls'], 1e-4, 1e-4)
    close(reg_l[0], g7['reg_branch'], 1e-4, 1e-4)
    close(reg_l[1], g7['reg'], 1e-4, 1e-4)


def test_g11_selsa_head_training_step(O):
    """Losses and every parameter gradient of one SELSA-head training step against the reference modules' own
    loss() + backward() (G11): small tensors element for element, large ones by sum / abs-sum / a strided sample."""
    g = gold('g11_selsa_train')
    labels, lw, bt, bw = C.head_train_case()
    losses, grads, dx = O.selsa_head_train_step(C.roi_feat_input(), S.synth_state_dict('selsa'), dict(start=32, length=32), 32, 3,
                                                labels, lw, bt, bw)
    for k in ('loss_cls', 'loss_bbox', 'acc'):
        close(losses[k], g[k], 1e-5, 1e-6)
    close(dx.reshape(-1)[::4099], g['d_feats_sample'], 1e-4, 1e-7)
    assert abs(float(dx.double().abs().sum()) - float(g['d_feats_abs'])) <= 1e-4 * float(g['d_feats_abs'])
    seen = 0
    for name, gr in grads.items():
        key = name.replace('.', '__')
        if 'k_data_fc' in name and name.endswith('bias'):  # analytically zero (softmax is shift-invariant): round-off only
            assert float(gr.double().abs().sum()) <= 1e-4 * float(g['abs__' + key.replace('k_data_fc', 'q_data_fc')]), name
            seen += 1
            continue
        assert abs(float(gr.double().abs().sum()) - float(g['abs__' + key])) <= 1e-4 * float(g['abs__' + key]) + 1e-9, name
        if 'full__' + key in g.files:
            close(gr, g['full__' + key], 1e-4, 1e-6)
        else:
            close(gr.reshape(-1)[::4099], g['sample__' + key], 1e-4, 1e-7)
        seen += 1
    assert seen == 20  # fc_new_1/2, two relation stages (q, k, out), fc_cls, fc_reg: weights and biases


def _replay_keys(n, chosen):
    """Sampler keys under which the oracle's / the HIP path's "smallest keys win" rule picks exactly `chosen`:
    the reference drew its subset with a host-side numpy shuffle (random_sampler.py:19-35); the subset is the fixture."""
    keys = torch.ones(n)
    keys[torch.as_tensor(np.asarray(chosen)).long()] = 0.0
    return keys


def test_g12_training_targets(O):
    """Assigner, samplers, anchor_target, RPN loss, bbox_target and the OHEM loss against the reference's own classes (G12)."""
    g = gold('g12_targets')
    tc = C.target_case()
    gt_b, gt_l = tc['gt_bboxes'], tc['gt_labels']
    anchors = O.grid_anchors(O.gen_base_anchors(16, [4, 8, 16, 32], [0.5, 1.0, 2.0]), (38, 63), 16)
    inside = O.anchor_inside_flags(anchors, (600, 1000, 3), 0)
    assert np.array_equal(inside.numpy(), g['inside'])
    a = C.RPN_TRAIN_CFG['assigner']
    gt_inds, max_ov = O.max_iou_assign(anchors[inside], gt_b, a['pos_iou_thr'], a['neg_iou_thr'], a['min_pos_iou'])
    assert np.array_equal(gt_inds.numpy(), g['rpn_gt_inds'])
    assert np.array_equal(max_ov.numpy(), g['rpn_max_overlaps'])
    assert (gt_inds == 3).sum() == 0 and (gt_inds == 5).sum() == 1 and float(max_ov[gt_inds == 5]) < 0.7   # both step-4 branches
    keys = _replay_keys(anchors.shape[0], np.nonzero(g['rpn_label_weights'] > 0)[0])
    lab, lw, bt, bw, npos, nneg = O.anchor_target_single(anchors, gt_b, (600, 1000, 3), keys, C.RPN_TRAIN_CFG)
    assert (npos, nneg) == (int(g['rpn_num_pos']), int(g['rpn_num_neg']))
    assert np.array_equal(lab.numpy(), g['rpn_labels']) and np.array_equal(lw.numpy(), g['rpn_label_weights'])
    assert np.array_equal(bw.numpy(), g['rpn_bbox_weights'])
    close(bt, g['rpn_bbox_targets'], 1e-6, 1e-7)
    cls, reg = tc['rpn_cls'].clone().requires_grad_(True), tc['rpn_reg'].clone().requires_grad_(True)
    lc, lb = O.rpn_loss(cls, reg, lab, lw, bt, bw, max(npos, 1) + max(nneg, 1))
    close(lc.detach(), g['loss_rpn_cls'], 1e-5, 1e-6)
    close(lb.detach(), g['loss_rpn_bbox'], 1e-5, 1e-6)
    (lc + lb).backward()
    close(cls.grad, g['d_rpn_cls'], 1e-5, 1e-8)
    close(reg.grad[reg.grad != 0], g['d_rpn_reg_nz'], 1e-5, 1e-8)
    # RCNN sampling + targets
    k = gt_b.shape[0]
    chosen = np.concatenate([g['rcnn_pos_inds'], g['rcnn_neg_inds']])
    samp = O.rcnn_assign_sample(tc['proposals'], gt_b, gt_l, _replay_keys(k + tc['proposals'].shape[0], chosen), C.RCNN_TRAIN_CFG)
    assert np.array_equal(samp['gt_inds'][k:].numpy(), g['rcnn_gt_inds'])
    assert np.array_equal(samp['pos_inds'].numpy(), g['rcnn_pos_inds']) and np.array_equal(samp['neg_inds'].numpy(), g['rcnn_neg_inds'])
    rois = torch.cat([samp['bboxes'][samp['pos_inds']], samp['bboxes'][samp['neg_inds']]])
    assert np.array_equal(rois.numpy(), g['rcnn_rois'])
    labels, label_w, bbox_t, bbox_w = O.bbox_target_single(samp, gt_b, gt_l)
    assert np.array_equal(labels.numpy(), g['rcnn_labels']) and np.array_equal(label_w.numpy(), g['rcnn_label_weights'])
    assert np.array_equal(bbox_w.numpy(), g['rcnn_bbox_weights'])
    close(bbox_t, g['rcnn_bbox_targets'], 1e-5, 1e-6)
    # OHEM: the ranking is deterministic (top-k of the row losses), no replay keys needed
    n = labels.shape[0]
    cs, bp = tc['cls_score'][:n].clone().requires_grad_(True), tc['bbox_pred'][:n].clone().requires_grad_(True)
    oh = C.RCNN_TRAIN_CFG['ohem']
    losses, opos, oneg = O.ohem_loss(cs, bp, labels, bbox_t, oh['num'], oh['pos_fraction'], oh['neg_pos_ub'])
    assert np.array_equal(opos.numpy(), g['ohem_pos_inds']) and np.array_equal(oneg.numpy(), g['ohem_neg_inds'])
    close(losses['loss_cls'].detach(), g['ohem_loss_cls'], 1e-5, 1e-6)
    close(losses['loss_bbox'].detach(), g['ohem_loss_bbox'], 1e-5, 1e-6)
    close(losses['acc'], g['ohem_acc'], 1e-5, 1e-6)
    (losses['loss_cls'] + losses['loss_bbox']).backward()
    close(cs.grad, g['ohem_d_cls'], 1e-5, 1e-8)
    close(bp.grad, g['ohem_d_reg'], 1e-5, 1e-8)


def test_sampler_keys_pick_the_smallest_with_index_ties(O):
    """The key rule itself: fewer candidates than expected -> all of them; more -> the smallest keys, ties by lower index;
    neg_pos_ub caps the negatives; output sorted."""
    cls = torch.tensor([1, 0, 0, 2, -1, 0, 1, 0, 0, 3])
    keys = torch.tensor([.5, .9, .1, .5, 0., .1, .2, .1, .7, .5])
    pos, neg = O.sample_pos_neg(cls, keys, num=6, pos_fraction=0.5)
    assert pos.tolist() == [0, 3, 6] and neg.tolist() == [2, 5, 7]
    pos, neg = O.sample_pos_neg(cls, keys, num=4, pos_fraction=0.5)
    assert pos.tolist() == [0, 6] and neg.tolist() == [2, 5]
    pos, neg = O.sample_pos_neg(cls, keys, num=10, pos_fraction=0.2, neg_pos_ub=1.5)
    assert pos.tolist() == [0, 6] and neg.tolist() == [2, 5, 7]


def test_g13_hard_proposal_mining(O):
    """The oracle's masked arg-reductions against the reference's own hardest_proposal_mining (G13), on a case with a
    single-key class and a query class without keys; the best-vs-second gap of the case is far above f32 round-off."""
    g = gold('g13_mining')
    labels, all_labels, aff = C.mining_case()
    anchors, pos, neg, bg2 = O.hardest_proposal_mining(labels, all_labels, aff)
    assert np.array_equal(anchors.numpy(), g['anchor_idx'])
    assert np.array_equal(pos.numpy(), g['hardest_pos_idx']) and np.array_equal(neg.numpy(), g['hardest_neg_idx'])
    assert float(g['min_gap']) > 1e-4
    assert bg2.shape == (labels.numel(), 2) and bool((all_labels[bg2[labels == 0]] != 0).all())


def test_g15_hvr_head_training_forward_and_backward(O):
    """G15: the reference's own HRNMPBBoxHead.forward (training, dynamic=False, as hnmb_rcnn.py:438 calls it) + HRNMPBBoxHead.loss +
    backward() on three videos of three frames, with a recording stub where its tree lacks TripletNonLocalLoss (the stub returns a
    connected zero): both branches' logits and box deltas, the six loss outputs, what the head hands the triplet loss (q / k
    projections, the mined index triple), the RoI-feature gradients and eleven parameter gradients (sum, abs-sum, strided sample)
    pin oracle.hvr_head_forward_train / hvr_head_loss -- everything of the HVR training forward except the triplet term's value."""
    g = gold('g15_hvr_train')
    feats, cur, labels, lw, bt, bw = C.hvr_train_case()
    sd = S.synth_state_dict('hvr')
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith('bbox_head.')}
    fg = [f.clone().requires_grad_(True) for f in feats]
    rec = {}
    cls, reg, extra = O.hvr_head_forward_train(fg, leaf, cur, labels, 16, 9, 3, record=rec)
    for got, key in ((cls[0], 'cls_branch'), (cls[1], 'cls'), (reg[0], 'reg_branch'), (reg[1], 'reg')):
        close(got.detach(), g[key], 1e-4, 1e-5)
    losses = O.hvr_head_loss(cls, reg, labels, lw, bt, bw)
    for k in ('loss_cls_1', 'loss_bbox_1', 'acc_1', 'loss_cls_2', 'loss_bbox_2', 'acc_2'):
        close(losses[k].detach(), g[k], 1e-5, 1e-6)
    # what the reference hands its triplet loss
    assert tuple(rec['q'].shape) == tuple(int(x) for x in g['trip_q_shape'])
    assert abs(float(rec['q'].double().abs().sum()) - float(g['trip_q_abs'])) <= 1e-4 * float(g['trip_q_abs'])
    assert abs(float(rec['k'].double().abs().sum()) - float(g['trip_k_abs'])) <= 1e-4 * float(g['trip_k_abs'])
    assert np.array_equal(rec['anchors'].numpy(), g['trip_anchor_idx'])
    assert np.array_equal(rec['second'].numpy(), g['trip_second_idx']) and np.array_equal(rec['third'].numpy(), g['trip_third_idx'])
    assert 'loss_trip' in extra          # (the stand-in's value: unpinned, and left out of the sum below as the stub's zero is)
    sum(v for k, v in losses.items() if k.startswith('loss')).backward()
    for v_i, f in enumerate(fg):
        want_abs = float(g['d_feats%d_abs' % v_i])
        assert abs(float(f.grad.double().abs().sum()) - want_abs) <= 1e-4 * want_abs, v_i
        assert abs(float(f.grad.double().sum()) - float(g['d_feats%d_sum' % v_i])) <= 1e-4 * want_abs, v_i
    seen = 0
    for key in [k[len('abs__'):] for k in g.files if k.startswith('abs__')]:
        gr = leaf['bbox_head.' + key.replace('__', '.')].grad
        want_abs = float(g['abs__' + key])
        assert abs(float(gr.double().abs().sum()) - want_abs) <= 1e-4 * want_abs + 1e-9, key
        close(gr.reshape(-1)[::4099], g['sample__' + key], 1e-4, 1e-6 * max(1.0, want_abs / gr.numel()))
        seen += 1
    assert seen == 11


def test_roi_align_f64_restatement_equals_the_c_restatement(O):
    """oracle._roi_align_f64 (torch, float64: used by the f64 noise-floor run of the whole path) against oracle_ref.c on the same
    boxes: interior, protruding, degenerate and out-of-image RoIs; the difference is f32 evaluation order only."""
    g = torch.Generator().manual_seed(31)
    feat = torch.randn((2, 6, 19, 31), generator=g)
    rois = torch.tensor([[0, 10., 12., 200., 150.], [1, -30., -20., 90., 60.], [0, 400., 250., 520., 330.], [1, 37.5, 41.25, 37.5, 41.25],
                         [0, 0., 0., 495., 303.], [1, 700., 700., 900., 900.], [0, 100., 50., 90., 40.]])
    a = O.roi_align(feat, rois, 7, 1.0 / 16, 2)
    b = O.roi_align(feat.double(), rois.double(), 7, 1.0 / 16, 2)
    assert b.dtype == torch.float64 and a.shape == b.shape
    close(a, b.float(), 1e-5, 1e-5)


def test_ingest_oracle_closed_form_cases(O):
    """OpenCV is not in the image, so the resize restatement is pinned by cases with known answers: identity, an exact 2x
    reduction (every output = the rounded mean of a 2x2 block), constants under any scale, border replication when
    upscaling, and the pipeline's shapes / meta for the three VID frame sizes."""
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    assert np.array_equal(O.cv2_resize_linear_u8(img, (37, 53)), img)
    even = rng.randint(0, 256, (40, 64, 3)).astype(np.uint8)
    half = O.cv2_resize_linear_u8(even, (20, 32))
    blocks = even.reshape(20, 2, 32, 2, 3).astype(np.int64)
    s = blocks.sum(axis=(1, 3))
    assert np.abs(half.astype(np.int64) * 4 - s).max() <= 2 and np.array_equal(half, ((s + 2) >> 2).astype(np.uint8))
    const = np.full((23, 31, 3), 137, dtype=np.uint8)
    for hw in ((46, 62), (11, 17), (23, 100)):
        assert (O.cv2_resize_linear_u8(const, hw) == 137).all()
    up = O.cv2_resize_linear_u8(img, (74, 106))
    assert np.array_equal(up[0, 0], img[0, 0]) and np.array_equal(up[-1, -1], img[-1, -1])     # (0.5 * 0.5 - 0.5 < 0: clamped tap)
    assert up.min() >= img.min() and up.max() <= img.max()
    for (h, w), want in (((720, 1280), (563, 1000, 576, 1008)), ((360, 480), (600, 800, 608, 800)), ((600, 1000), (600, 1000, 608, 1008))):
        out, meta = O.ingest_frame(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        assert meta['img_shape'][:2] == want[:2] and meta['pad_shape'][:2] == want[2:] and tuple(out.shape) == (1, 3) + want[2:]
        assert float(out[0, :, want[0]:, :].abs().sum()) == 0 and float(out[0, :, :, want[1]:].abs().sum()) == 0
    frame = rng.randint(0, 256, (600, 1000, 3)).astype(np.uint8)
    out, meta = O.ingest_frame(frame)
    assert meta['scale_factor'] == 1.0
    want = frame.astype(np.float32) - np.array([103.06, 115.90, 123.15], dtype=np.float32)
    assert np.array_equal(out[0, :, :600, :1000].numpy(), want.transpose(2, 0, 1))


def test_g8_det_readout(O):
    g = gold('g8_det')
    rois, cls, reg = C.det_case()
    cfg = dict(score_thr=0.001, nms=dict(type='nms', iou_thr=0.3), max_per_img=300)
    bb, sc = O.get_det_bboxes(rois, cls, reg, (600, 1000, 3), 1.0, False, None)
    close(bb, g['bboxes'], 0, 0)
    close(sc, g['scores'], 1e-6, 1e-7)
    db, dl = O.get_det_bboxes(rois, cls, reg, (600, 1000, 3), 1.0, True, cfg)
    assert dl.tolist() == g['det_labels'].tolist()
    close(db, g['det_bboxes'], 1e-6, 1e-6)
    cfg100 = dict(cfg, max_per_img=100)
    db, dl = O.get_det_bboxes(rois, cls, reg, (600, 1000, 3), 2.0, True, cfg100)
    assert dl.tolist() == g['det_labels_top100'].tolist()
    close(db, g['det_bboxes_top100'], 1e-6, 1e-6)


def test_g9_backbone_small(O):
    g = gold('g9_backbone_small')
    sd = S.synth_state_dict('hvr')
    with torch.no_grad():
        c4 = O.resnet_c4(C.small_image(), sd)
        c5 = O.shared_head(c4, sd)
        rc, rr = O.rpn_forward(c4, sd)
    close(c4, g['c4'], 1e-4, 1e-3)
    close(c5, g['c5'], 1e-4, 1e-4)
    close(rc, g['rpn_cls'], 1e-4, 1e-4)
    close(rr, g['rpn_reg'], 1e-4, 1e-4)


@pytest.mark.timeout(600)
def test_g10_config1_end_to_end(O):
    """configs[0]: 1 key + 2 reference frames of 600x1000, 32 proposals, CPU forward."""
    g = gold('g10_config1')
    T, key = 3, 1
    torch.set_num_threads(os.cpu_count() or 1)
    imgs = [S.synth_frame(i) for i in range(T)]
    metas = [S.synth_meta() for _ in range(T)]
    rpn_cfg = dict(O.RPN_TEST_CFG, nms_post=32, max_num=32)
    sd = S.synth_state_dict('hvr')
    with torch.no_grad():
        c4 = [O.resnet_c4(im, sd) for im in imgs]
        res, inter = O.window_forward(c4, metas, sd, 'hvr', key, 32, 3, rpn_cfg=rpn_cfg, return_intermediates=True)
    xcat = torch.cat(c4, 0)
    close(xcat[:, :8, 10:14, 20:24], g['c4_slice'], 1e-4, 1e-3)
    close(inter['c5'][:, :8, 10:14, 20:24], g['c5_slice'], 1e-4, 1e-4)
    close(torch.stack(inter['proposals']), g['proposals'], 1e-4, 2e-2)
    for b in range(2):
        close(inter['cls_scores'][b], g['hvr_cls_%d' % b], 1e-3, 1e-3)
        close(inter['bbox_preds'][b], g['hvr_reg_%d' % b], 1e-3, 1e-3)
        db, dl = inter['dets'][b]
        assert dl.tolist() == g['hvr_det_labels_%d' % b].tolist()  # class indices exact
        close(db, g['hvr_det_bboxes_%d' % b], 1e-3, 1e-3)           # boxes / scores within 1e-3
    # SELSA head on the same window
    sd_s = S.synth_state_dict('selsa')
    with torch.no_grad():
        res_s, inter_s = O.window_forward(c4, metas, sd_s, 'selsa', key, 32, 3, rpn_cfg=rpn_cfg, return_intermediates=True)
    close(inter_s['cls_scores'][0], g['selsa_cls'], 1e-3, 1e-3)
    db, dl = inter_s['dets'][0]
    assert dl.tolist() == g['selsa_det_labels'].tolist()
    close(db, g['selsa_det_bboxes'], 1e-3, 1e-3)
