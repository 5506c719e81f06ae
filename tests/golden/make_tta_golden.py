"""Generates tests/golden/g18_merge_augs.npz and g19_tta_config1.npz by running the REFERENCE's own test-time-augmentation code
(build container only; needs the reference tree at make_golden.REF and oracle/_ref):

    python tests/golden/make_tta_golden.py            # HVR_GOLDEN_ONLY=g18 / g19 rewrites only that fixture

It uses the stub loader of make_golden.py (`install_reference`, untouched) and loads on top of it, where they lie,
mmdet/core/post_processing/merge_augs.py (with the reference's compiled nms_cpu) and
mmdet/models/detectors/{base,test_mixins,two_stage,hnmb_rcnn}.py, so that G19 is HNMBRCNN.forward_feat_aug / aug_test_bboxes
themselves, called as plain functions on an object that carries the reference's modules.  Nothing of the reference is copied:
the script executes it and stores arrays.  RoIAlign has no CPU path in the reference (roi_align.py:27-28): the oracle's
restatement stands in, as in G10 (`roi_align: "oracle"`).

Every merge case satisfies the margin conditions of tests/tta_refs.py (asserted here, by the reference's numbers alone): no pair of
the union within 1e-4 of nms_thr, no equal surviving scores, a score gap above 1e-5 at the max_num cut; G19 also keeps that IoU
margin at the final multiclass NMS.  A seed that fails a condition is replaced by the next one; the seed used is stored.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG  # noqa: E402  (pins the CPU numeric path on import)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import tta_refs as R  # noqa: E402

AttrDict = MG.AttrDict


def install_tta(ref):
    """merge_augs.py and the detector classes on top of install_reference()'s stub packages."""
    core = sys.modules['mmdet.core']
    sys.modules['mmdet.core.bbox'].bbox_mapping_back = ref.tr.bbox_mapping_back
    ma = MG._load('mmdet.core.post_processing.merge_augs', 'mmdet/core/post_processing/merge_augs.py')
    core.merge_aug_proposals, core.merge_aug_bboxes, core.merge_aug_masks = ma.merge_aug_proposals, ma.merge_aug_bboxes, ma.merge_aug_masks
    core.bbox_mapping_back = ref.tr.bbox_mapping_back
    return ma


def install_detectors():
    pm = MG._pkg('pycocotools')
    pm.mask = MG._pkg('pycocotools.mask')
    mmcv = sys.modules['mmcv']
    mmcv.imshow_det_bboxes = None
    sys.modules['mmdet.utils'].print_log = lambda *a, **k: None
    core = sys.modules['mmdet.core']
    for n in ('tensor2imgs', 'get_classes', 'bbox2result', 'bbox2roi', 'build_assigner', 'build_sampler', 'bbox_overlaps'):
        if not hasattr(core, n):
            setattr(core, n, None)
    tr = sys.modules['mmdet.core.bbox.transforms']
    core.bbox2result, core.bbox2roi, core.bbox_mapping = tr.bbox2result, tr.bbox2roi, tr.bbox_mapping
    MG._pkg('mmdet.models.detectors')
    MG._load('mmdet.models.detectors.base', 'mmdet/models/detectors/base.py')
    MG._load('mmdet.models.detectors.test_mixins', 'mmdet/models/detectors/test_mixins.py')
    MG._load('mmdet.models.detectors.two_stage', 'mmdet/models/detectors/two_stage.py')
    return MG._load('mmdet.models.detectors.hnmb_rcnn', 'mmdet/models/detectors/hnmb_rcnn.py').HNMBRCNN


def metas_arrays(metas):
    return dict(img_h=np.array([m['img_shape'][0] for m in metas], np.int32), img_w=np.array([m['img_shape'][1] for m in metas], np.int32),
                scale=np.array([m['scale_factor'] for m in metas], np.float64), flip=np.array([m['flip'] for m in metas], np.bool_))


MERGE_CASES = [   # name, scales, flip, boxes per aug, max_num, short = (aug, rows) or None
    ('a2_300', (1.0,), True, 300, 300, None),
    ('a4_300', (1.0, 0.8), True, 300, 300, None),
    ('a2_32', (1.0,), True, 32, 32, None),
    ('a4_32', (1.0, 0.8), True, 32, 32, None),
    ('a4_300_short', (1.0, 0.8), True, 300, 300, (2, 187)),
]
NMS_THR = 0.7


def make_g18(ref, ma):
    out = {}
    # ---- bbox_flip / bbox_mapping / bbox_mapping_back ----
    g = torch.Generator().manual_seed(1800)
    x1, y1 = torch.rand(64, generator=g) * 700, torch.rand(64, generator=g) * 400
    boxes = torch.stack([x1, y1, x1 + 1 + torch.rand(64, generator=g) * 290, y1 + 1 + torch.rand(64, generator=g) * 190], 1).float()
    shape = (480, 800, 3)
    out.update(tr_boxes=boxes, tr_img_shape=np.array(shape, np.int32), tr_scale=np.float64(0.8),
               tr_flip=ref.tr.bbox_flip(boxes, shape), tr_flip8=ref.tr.bbox_flip(boxes.reshape(32, 8), shape),
               tr_map=ref.tr.bbox_mapping(boxes, shape, 0.8, False), tr_map_flip=ref.tr.bbox_mapping(boxes, shape, 0.8, True),
               tr_back=ref.tr.bbox_mapping_back(boxes, shape, 0.8, False), tr_back_flip=ref.tr.bbox_mapping_back(boxes, shape, 0.8, True))
    # ---- merge_aug_proposals ----
    names = []
    for i, (name, scales, flip, n, max_num, short) in enumerate(MERGE_CASES):
        metas = R.aug_metas((600, 1000), scales, flip)
        seed, props = R.random_case(1810 + 20 * i, metas, n, NMS_THR, max_num, short=short)
        assert R.margins_ok(props, metas, NMS_THR, max_num)
        cfg = AttrDict(nms_thr=NMS_THR, max_num=max_num)
        merged = ma.merge_aug_proposals([p.clone() for p in props], metas, cfg)
        mine, src = R.merge_aug_proposals(props, metas, NMS_THR, max_num, return_index=True)
        assert torch.equal(mine, merged), 'tests/tta_refs.py does not restate merge_aug_proposals bit for bit (%s)' % name
        names.append(name)
        out['mp_%s_seed' % name] = np.int64(seed)
        out['mp_%s_max_num' % name] = np.int32(max_num)
        for k, v in metas_arrays(metas).items():
            out['mp_%s_%s' % (name, k)] = v
        for a, p in enumerate(props):
            out['mp_%s_props_%d' % (name, a)] = p
        out['mp_%s_merged' % name], out['mp_%s_src' % name] = merged, src
        print('g18 %s: seed %d, %d boxes -> %d merged' % (name, seed, sum(p.shape[0] for p in props), merged.shape[0]))
    out['mp_names'] = np.array(names)
    out['mp_nms_thr'] = np.float64(NMS_THR)
    # ---- merge_aug_bboxes, 31 classes ----
    for name, scales, Rn in (('a4', (1.0, 0.8), 300), ('a2', (1.0,), 32)):
        metas = R.aug_metas((600, 1000), scales, True)
        bxs, scs = R.random_dets(1890, metas, Rn, 31)
        mb, ms = ma.merge_aug_bboxes(bxs, scs, [[m] for m in metas], None)
        for k, v in metas_arrays(metas).items():
            out['mb_%s_%s' % (name, k)] = v
        out['mb_%s_boxes' % name], out['mb_%s_scores' % name] = torch.stack(bxs), torch.stack(scs)
        out['mb_%s_merged_boxes' % name], out['mb_%s_merged_scores' % name] = mb, ms
        out['mb_%s_merged_scores_only' % name] = ma.merge_aug_scores(scs)
    MG.save('g18_merge_augs', **out)


# ------------------------------------------------------------------------------------------------------------------ G19
G19_SCALES = ((1000, 600), (800, 480))     # img_scale -> scale_factor 1.0 / 0.8 on the 600 x 1000 synthetic frames
G19_T, G19_KEY, G19_MX = 3, 1, 32


def g19_frames(S, frame_seed=0):
    """Per augmentation (scale outer, flip inner) the T frames [1,3,pad_h,pad_w] and their metas -- what the test rebuilds."""
    imgs, metas = [], []
    for (long_edge, short_edge) in G19_SCALES:
        s = short_edge / 600.0
        ih, iw = int(600 * s + 0.5), int(1000 * s + 0.5)
        ph, pw = -(-ih // 16) * 16, -(-iw // 16) * 16
        for flip in (False, True):
            fr = []
            for i in range(G19_T):
                im = S.synth_frame(i, seed=frame_seed, img_hw=(ih, iw), pad_hw=(ph, pw))
                if flip:
                    im = im.clone()
                    im[:, :, :ih, :iw] = torch.flip(im[:, :, :ih, :iw], dims=[3])
                fr.append(im)
            imgs.append(fr)
            metas.append([dict(ori_shape=(600, 1000, 3), img_shape=(ih, iw, 3), pad_shape=(ph, pw, 3), scale_factor=float(s), flip=flip)
                          for _ in range(G19_T)])
    return imgs, metas


def make_g19(ref, ma):
    import collections
    import collections.abc
    import torch.nn as nn
    from hvrnet_amd import synthetic as S
    from oracle import hvr_oracle as O
    if not hasattr(collections, 'Sequence'):       # hnmb_rcnn.py:106 (collections.Sequence -> collections.abc)
        collections.Sequence = collections.abc.Sequence
    HNMBRCNN = install_detectors()
    mod = sys.modules['mmdet.models.detectors.hnmb_rcnn']
    sd = S.synth_state_dict('hvr')
    norm_cfg = dict(type='BN', requires_grad=False)
    backbone = ref.ResNet(depth=101, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), frozen_stages=1,
                          style='caffe', norm_eval=True, norm_cfg=norm_cfg)
    backbone.eval()
    backbone.load_state_dict(MG._sub_state(sd, 'backbone'), strict=True)
    shared = ref.ResLayer(depth=101, stage=3, stride=1, dilation=2, style='caffe', norm_eval=True, norm_cfg=norm_cfg, external_conv=True)
    shared.eval()
    shared.load_state_dict(MG._sub_state(sd, 'shared_head'), strict=True)
    rpn = ref.RPNHead(in_channels=1024, feat_channels=512, anchor_scales=[4, 8, 16, 32], anchor_ratios=[0.5, 1.0, 2.0],
                      anchor_strides=[16], target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0],
                      loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                      loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)).eval()
    rpn.load_state_dict(MG._sub_state(sd, 'rpn_head'), strict=True)
    common = dict(with_avg_pool=False, in_channels=256, fc_feat_dim=1024, roi_feat_size=7, num_classes=31,
                  target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2], reg_class_agnostic=True,
                  loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                  loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    hvr = ref.HRNMPBBoxHead(sampler_num=G19_MX, t_dim=G19_T, imgs_per_video=3, **common).eval()
    hvr.load_state_dict(MG._sub_state(sd, 'bbox_head'), strict=True)

    class OracleRoIAlign(object):      # RoIAlign has no CPU path in the reference: the oracle's restatement, as in G10
        num_inputs = 1

        def __call__(self, feats, rois):
            return O.roi_align(feats[0], rois, 7, 1.0 / 16, 2)

    det = HNMBRCNN.__new__(HNMBRCNN)
    nn.Module.__init__(det)
    det.shared_head, det.rpn_head, det.bbox_head = shared, rpn, hvr
    det.bbox_roi_extractor = OracleRoIAlign()
    det.feat_from_shared_head, det.key_dim = True, G19_KEY
    det.test_cfg = AttrDict(rpn=AttrDict(nms_across_levels=False, nms_pre=6000, nms_post=G19_MX, max_num=G19_MX, nms_thr=NMS_THR, min_bbox_size=0),
                            rcnn=AttrDict(score_thr=0.001, nms=AttrDict(type='nms', iou_thr=0.3), max_per_img=300))
    det.eval()

    rec = dict(props=[], merged=[], aug_boxes=[], aug_scores=[], mboxes=[], mscores=[])
    real_mp, real_mb, real_nms = ma.merge_aug_proposals, ma.merge_aug_bboxes, mod.multiclass_nms

    def rec_mp(aug_proposals, img_metas, cfg):
        out = real_mp(aug_proposals, img_metas, cfg)
        rec['props'].append([p.clone() for p in aug_proposals])
        rec['merged'].append(out.clone())
        return out

    def rec_mb(aug_bboxes, aug_scores, img_metas, cfg):
        mb, ms = real_mb(aug_bboxes, aug_scores, img_metas, cfg)
        rec['aug_boxes'].append(torch.stack(aug_bboxes))
        rec['aug_scores'].append(torch.stack(aug_scores))
        rec['mboxes'].append(mb.clone())
        rec['mscores'].append(ms.clone())
        return mb, ms

    mod.merge_aug_proposals, mod.merge_aug_bboxes = rec_mp, rec_mb
    for frame_seed in range(16):        # the first frame seed whose RPN output satisfies the margin conditions
        imgs, metas = g19_frames(S, frame_seed)
        A = len(imgs)
        with torch.no_grad():
            c4 = [[backbone(im)[0] for im in imgs[a]] for a in range(A)]
            per_aug = [det.simple_test_rpn([torch.cat(c4[a], 0)], metas[a], det.test_cfg.rpn) for a in range(A)]
        why = []
        ok = all(R.margins_ok([per_aug[a][t] for a in range(A)], [metas[a][t] for a in range(A)], NMS_THR, G19_MX, why) for t in range(G19_T))
        print('g19 frame seed %d: %s' % (frame_seed, 'ok' if ok else why[-1]))
        if ok:
            break
    else:
        raise SystemExit('g19: no frame seed satisfies the margin conditions')
    with torch.no_grad():
        x = [[c4[a][t] for a in range(A)] for t in range(G19_T)]
        img_meta = [[metas[a][t] for a in range(A)] for t in range(G19_T)]
        results = det.forward_feat_aug(x=x, img_meta=img_meta, rescale=True)
        dets, labels = det.aug_test_bboxes([[shared(torch.cat(c4[a], 0))] for a in range(A)], metas, rec['merged'][:G19_T], det.test_cfg.rcnn)
    mod.merge_aug_proposals, mod.merge_aug_bboxes = real_mp, real_mb
    # margin conditions, on the reference's numbers alone (the frames are seeded by synthetic.synth_frame)
    for t in range(G19_T):
        assert all(p.shape[0] == G19_MX for p in rec['props'][t]) and rec['merged'][t].shape[0] == G19_MX
        assert R.margins_ok(rec['props'][t], [metas[a][t] for a in range(A)], NMS_THR, G19_MX), 'frame %d fails the margin conditions' % t
    for b in range(2):
        assert not np.any(np.abs(R.pair_ious(rec['mboxes'][b]) - 0.3) <= R.IOU_MARGIN), 'branch %d: a pair sits on the final NMS threshold' % b
    out = dict(composed=np.bool_(False), roi_align=np.array('oracle'), frame_seed=np.int64(frame_seed), key_dim=np.int32(G19_KEY),
               img_scale=np.array(G19_SCALES, np.int32), props=torch.stack([torch.stack(rec['props'][t]) for t in range(G19_T)]).permute(1, 0, 2, 3),
               merged=torch.stack(rec['merged'][:G19_T]))
    for k, v in metas_arrays([metas[a][0] for a in range(A)]).items():
        out[k] = v
    out['pad_h'] = np.array([metas[a][0]['pad_shape'][0] for a in range(A)], np.int32)
    out['pad_w'] = np.array([metas[a][0]['pad_shape'][1] for a in range(A)], np.int32)
    for b in range(2):
        out['aug_boxes_%d' % b], out['aug_scores_%d' % b] = rec['aug_boxes'][b], rec['aug_scores'][b]
        out['merged_boxes_%d' % b], out['merged_scores_%d' % b] = rec['mboxes'][b], rec['mscores'][b]
        out['det_bboxes_%d' % b], out['det_labels_%d' % b] = dets[b], labels[b]
        got = np.concatenate([r for r in results[b]], 0)
        order = np.argsort(labels[b].numpy(), kind='stable')
        assert np.array_equal(got, dets[b].numpy()[order]), 'forward_feat_aug and aug_test_bboxes on its merged proposals disagree'
    out['c4_checksum'] = np.array([[c4[a][t].double().sum().item() for t in range(G19_T)] for a in range(A)])
    MG.save('g19_tta_config1', **out)


def main():
    import warnings
    warnings.filterwarnings('ignore')
    torch.set_num_threads(MG.numerics.THREADS)
    ref = MG.install_reference()
    ma = install_tta(ref)
    only = MG.ONLY
    if not only or any(t.startswith('g18') for t in only):
        make_g18(ref, ma)
    if not only or any(t.startswith('g19') for t in only):
        make_g19(ref, ma)


if __name__ == '__main__':
    main()
