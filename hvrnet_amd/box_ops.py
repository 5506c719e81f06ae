"""Box utilities with the reference's names and argument meaning (mmdet/core).

  AnchorGenerator      mmdet/core/anchor/anchor_generator.py:4-98   (host; constant per shape)
  delta2bbox           mmdet/core/bbox/transforms.py:34-111          (device kernel)
  bbox2roi             mmdet/core/bbox/transforms.py:149-168         (memory plumbing)
  bbox2result          mmdet/core/bbox/transforms.py:181-199         (D2H + split per class)
  multiclass_nms       mmdet/core/post_processing/bbox_nms.py:6-66   (device kernels; nms_cfg type 'nms' or 'soft_nms')
  bbox_flip / bbox_mapping / bbox_mapping_back   mmdet/core/bbox/transforms.py:114-146          (device kernels)
  merge_aug_proposals / merge_aug_bboxes / merge_aug_scores   mmdet/core/post_processing/merge_augs.py:8-77   (device kernels)
"""
import numpy as np
import torch

from . import native


class AnchorGenerator(object):
    """Base anchors are 12 numbers: they are computed on the host and handed to the RPN kernel,
    which derives every grid anchor on the fly (the reference rebuilds a [28 728, 4] tensor per call,
    anchor_head.py:258-263)."""

    def __init__(self, base_size, scales, ratios, scale_major=True, ctr=None):
        self.base_size = base_size
        self.scales = torch.Tensor(scales)
        self.ratios = torch.Tensor(ratios)
        self.scale_major = scale_major
        self.ctr = ctr
        self.base_anchors = self.gen_base_anchors()

    @property
    def num_base_anchors(self):
        return self.base_anchors.size(0)

    def gen_base_anchors(self):
        w = h = self.base_size
        x_ctr, y_ctr = (0.5 * (w - 1), 0.5 * (h - 1)) if self.ctr is None else self.ctr
        h_ratios = torch.sqrt(self.ratios)
        w_ratios = 1 / h_ratios
        if self.scale_major:
            ws = (w * w_ratios[:, None] * self.scales[None, :]).view(-1)
            hs = (h * h_ratios[:, None] * self.scales[None, :]).view(-1)
        else:
            ws = (w * self.scales[:, None] * w_ratios[None, :]).view(-1)
            hs = (h * self.scales[:, None] * h_ratios[None, :]).view(-1)
        return torch.stack([x_ctr - 0.5 * (ws - 1), y_ctr - 0.5 * (hs - 1), x_ctr + 0.5 * (ws - 1), y_ctr + 0.5 * (hs - 1)],
                           dim=-1).round()

    def grid_anchors(self, featmap_size, stride=16, device='cuda'):
        """(y, x, anchor)-ordered grid; kept for API parity (the fused RPN kernel does not need it)."""
        base = self.base_anchors.to(device)
        feat_h, feat_w = featmap_size
        sx = torch.arange(0, feat_w, device=device) * stride
        sy = torch.arange(0, feat_h, device=device) * stride
        xx = sx.repeat(len(sy))
        yy = sy.view(-1, 1).repeat(1, len(sx)).view(-1)
        shifts = torch.stack([xx, yy, xx, yy], dim=-1).type_as(base)
        return (base[None, :, :] + shifts[:, None, :]).view(-1, 4)


def delta2bbox(rois, deltas, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), max_shape=None, wh_ratio_clip=16 / 1000):
    """rois [N,4], deltas [N,4] (class-agnostic) -> boxes [N,4] on the device."""
    assert deltas.shape[1] == 4, 'only class-agnostic deltas are on the HVR hot path'
    n = rois.shape[0]
    rois5 = torch.cat([rois.new_zeros((n, 1)), rois[:, :4].float()], dim=1)
    logits = torch.cat([deltas.float().new_zeros((n, 1)), deltas.float()], dim=1).contiguous()
    _, boxes = native.det_decode(logits, 0, 1, 1, rois5, means, stds, max_shape, 0.0, wh_ratio_clip)
    return boxes


def bbox2roi(bbox_list):
    rois_list = []
    for img_id, bboxes in enumerate(bbox_list):
        if bboxes.size(0) > 0:
            img_inds = bboxes.new_full((bboxes.size(0), 1), img_id)
            rois_list.append(torch.cat([img_inds, bboxes[:, :4]], dim=-1))
        else:
            rois_list.append(bboxes.new_zeros((0, 5)))
    return torch.cat(rois_list, 0)


def bbox2result(bboxes, labels, num_classes):
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes - 1)]
    bboxes = bboxes.cpu().numpy()
    labels = labels.cpu().numpy()
    return [bboxes[labels == i, :] for i in range(num_classes - 1)]


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """Returns (bboxes [k,5], labels [k]) like the reference; one host read of k."""
    if score_factors is not None or multi_bboxes.shape[1] != 4:
        raise NotImplementedError('class-specific boxes / score_factors are outside the HVR hot path')
    nms_cfg_ = dict(nms_cfg)
    kind = nms_cfg_.get('type', 'nms')
    if kind not in ('nms', 'soft_nms'):
        raise NotImplementedError('nms type %r is outside the HVR hot path (nms, soft_nms)' % (kind,))
    if kind == 'soft_nms':
        native._soft_method(nms_cfg_.get('method', 'linear'))     # ValueError before any launch (nms_wrapper.py:88-90)
    R, nfg = multi_bboxes.shape[0], multi_scores.shape[1] - 1
    boxes, scores = multi_bboxes.float(), multi_scores.float()

    def run(cap):       # the operator the config names (bbox_nms.py:32-34), remaining keys handed on as the reference does
        return native.readout_nms(boxes, scores, score_thr, nms_cfg_, cap)

    if max_num < 0:
        # The reference's default max_num = -1 is not "no cap": `bboxes.shape[0] > max_num` is always true, so the survivors are
        # sorted by score and `inds[:max_num]` drops the last |max_num| of them (bbox_nms.py:55-59).  Reproduced as written:
        # count the survivors first (uncapped pass, class order), then cut to count + max_num in score order.
        dets, labels, n = run(max(R * nfg, 1))
        k = int(n.item()) + int(max_num)
        if k <= 0:
            return dets[:0], labels[:0]
        dets, labels, n = run(k)
        return dets[:k], labels[:k]
    dets, labels, n = run(max(int(max_num), 1))
    k = int(n.item())
    return dets[:k], labels[:k]


# ---- test-time augmentation (single frame, list inputs: the reference's signatures on the window kernels of csrc/tta.hip) ----
def _boxes2d(bboxes):
    if not torch.is_tensor(bboxes):
        raise NotImplementedError('the box mappings run on device tensors (no numpy / CPU fallback)')
    assert bboxes.shape[-1] % 4 == 0
    return bboxes.float().reshape(-1, 4)


def _scalar_scale(scale_factor):
    if not isinstance(scale_factor, (int, float)):
        raise NotImplementedError('per-axis scale_factor arrays are outside the HVR hot path')
    return float(scale_factor)


def bbox_mapping(bboxes, img_shape, scale_factor, flip):
    """Original image -> testing scale (transforms.py:131-136): boxes * scale_factor, then the horizontal flip."""
    b = _boxes2d(bboxes)
    if b.shape[0] == 0:
        return bboxes.float().clone()
    rows = torch.cat([b, b.new_zeros((b.shape[0], 1))], dim=1)[None]     # [1, n, 5]: one frame's (box, score) rows
    return native.map_aug_rois(rows, [img_shape[1]], [_scalar_scale(scale_factor)], [flip])[0, :, 1:].reshape(bboxes.shape)


def bbox_mapping_back(bboxes, img_shape, scale_factor, flip):
    """Testing scale -> original image (transforms.py:139-143): un-flip, then a division by scale_factor."""
    b = _boxes2d(bboxes)
    if b.shape[0] == 0:
        return bboxes.float().clone()
    out, _ = native.merge_aug_dets(b[None].contiguous(), b.new_zeros((1, b.shape[0], 1)), [img_shape[1]], [_scalar_scale(scale_factor)], [flip])
    return out.reshape(bboxes.shape)


def bbox_flip(bboxes, img_shape):
    """Horizontal flip (transforms.py:114-128), shape (..., 4 k)."""
    return bbox_mapping(bboxes, img_shape, 1.0, True)


def merge_aug_proposals(aug_proposals, img_metas, rpn_test_cfg):
    """merge_augs.py:8-44 for one frame: list of [n_a, 5] proposals, each in its augmentation's coordinates -> [k, 5] at
    original scale (mapped back, NMS at nms_thr with >=, descending score, first max_num).  One host read (k)."""
    n = [int(p.shape[0]) for p in aug_proposals]
    mx = max(max(n), 1)
    dev = aug_proposals[0].device
    props = torch.zeros((len(n), 1, mx, 5), dtype=torch.float32, device=dev)
    for a, p in enumerate(aug_proposals):
        props[a, 0, :n[a]] = p.float()
    counts = torch.tensor(n, dtype=torch.int32).view(-1, 1).to(dev)
    merged, cnt = native.merge_aug_proposals(props, counts, [m['img_shape'][1] for m in img_metas],
                                             [_scalar_scale(m['scale_factor']) for m in img_metas], [m['flip'] for m in img_metas],
                                             rpn_test_cfg['nms_thr'], rpn_test_cfg['max_num'])
    return merged[0, :int(cnt.item())]


def merge_aug_bboxes(aug_bboxes, aug_scores, img_metas, rcnn_test_cfg):
    """merge_augs.py:47-70: list of [n, 4] boxes (class-agnostic) + list of [n, ncls] scores (or None), img_metas a list of
    one-element lists -> (mean of the boxes mapped back, mean of the scores)."""
    boxes = torch.stack([b.float() for b in aug_bboxes], 0)
    if boxes.shape[2] != 4:
        raise NotImplementedError('class-specific boxes are outside the HVR hot path')
    scores = torch.stack([s.float() for s in aug_scores], 0) if aug_scores is not None else boxes.new_zeros(boxes.shape[:2] + (1,))
    mb, ms = native.merge_aug_dets(boxes, scores, [m[0]['img_shape'][1] for m in img_metas],
                                   [_scalar_scale(m[0]['scale_factor']) for m in img_metas], [m[0]['flip'] for m in img_metas])
    return mb if aug_scores is None else (mb, ms)


def merge_aug_scores(aug_scores):
    """merge_augs.py:73-78."""
    if not isinstance(aug_scores[0], torch.Tensor):
        return np.mean(aug_scores, axis=0)
    scores = torch.stack([s.float() for s in aug_scores], 0)
    flat = scores.reshape(scores.shape[0], -1, scores.shape[-1])
    A = flat.shape[0]
    _, ms = native.merge_aug_dets(flat.new_zeros((A, flat.shape[1], 4)), flat.contiguous(), [1.0] * A, [1.0] * A, [False] * A)
    return ms.reshape(scores.shape[1:])
