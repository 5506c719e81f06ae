"""Frame ingest on the device.

The reference's test pipeline (configs/faster_rcnn_r101_hrnmp_c5.py:193-201) is, per frame, on a DataLoader worker's CPU:
LoadImageFromFile (uint8 BGR) -> Resize(img_scale=(1000, 600), keep_ratio=True) = mmcv.imrescale -> cv2.resize(INTER_LINEAR)
-> RandomFlip(0) -> Normalize(mean, std, to_rgb) -> Pad(size_divisor=16) -> ImageToTensor -> Collect, then a 7 MB f32
host-to-device copy.  `FrameIngest` keeps the decode on the host and moves everything after it into one HIP kernel
(`hvr_ingest_frame`): the uint8 frame (1/4 of the bytes, before the upscale at that) is copied to the device and the
resized, mean-subtracted, zero-padded [1, 3, H, W] f32 tensor is written once, together with the img_meta the detector
needs (transforms.py:118-124,273-276: img_shape, pad_shape, scale_factor, flip).  `FrameIngestAug` is the MultiScaleFlipAug form of
the same pipeline (mmdet/datasets/pipelines/test_aug.py): several img_scales, each with and without a horizontal flip.
"""
import numpy as np
import torch

from . import native


def rescale_size(h, w, scale):
    """mmcv.imrescale's target size for scale = (long edge, short edge): factor = min(long / max(h, w), short / min(h, w)),
    new (w, h) = int(w * factor + 0.5), int(h * factor + 0.5).  -> (new_h, new_w, factor)."""
    max_long, max_short = max(scale), min(scale)
    factor = min(max_long / max(h, w), max_short / min(h, w))
    return int(h * float(factor) + 0.5), int(w * float(factor) + 0.5), factor


class FrameIngest(object):
    """Resize + RandomFlip + Normalize + Pad + ImageToTensor + Collect of the reference's test pipeline as one call.
    flip=True is RandomFlip with flip_ratio 1 (what MultiScaleFlipAug sets for its flipped half): the resized image is mirrored
    horizontally before the padding and img_meta['flip'] says so.

    frame: uint8 [H, W, 3] BGR -- a numpy array / CPU tensor (copied to `device`, asynchronously when pinned) or a tensor
    already on the device.  -> dict(img=[1, 3, pad_h, pad_w] f32 on the device, img_meta=dict(...))."""

    def __init__(self, img_scale=(1000, 600), mean=(103.06, 115.90, 123.15), std=(1.0, 1.0, 1.0), to_rgb=False, size_divisor=16,
                 keep_ratio=True, device='cuda:0', flip=False):
        if not keep_ratio:
            raise NotImplementedError('keep_ratio=False is not used by the HVRNet configs')
        self.img_scale, self.mean, self.std, self.to_rgb = tuple(img_scale), tuple(mean), tuple(std), bool(to_rgb)
        self.size_divisor, self.device, self.flip = int(size_divisor), device, bool(flip)

    def _to_device(self, frame):
        if isinstance(frame, np.ndarray):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError('expected a uint8 [H, W, 3] frame, got %s %s' % (frame.dtype, tuple(frame.shape)))
        if not frame.is_cuda:
            frame = frame.contiguous().to(self.device, non_blocking=True)
        return frame.contiguous()

    def geometry(self, h, w):
        """-> (new_h, new_w, pad_h, pad_w, scale_factor) of an h x w frame under this img_scale."""
        nh, nw, factor = rescale_size(h, w, self.img_scale)
        d = self.size_divisor
        return nh, nw, -(-nh // d) * d, -(-nw // d) * d, factor

    def meta(self, h, w):
        nh, nw, ph, pw, factor = self.geometry(h, w)
        return dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3), scale_factor=factor, flip=self.flip,
                    img_norm_cfg=dict(mean=np.array(self.mean, dtype=np.float32), std=np.array(self.std, dtype=np.float32),
                                      to_rgb=self.to_rgb))

    def __call__(self, frame):
        frame = self._to_device(frame)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        nh, nw, ph, pw, _ = self.geometry(h, w)
        img = native.ingest_frame(frame, (nh, nw), (ph, pw), self.mean, self.std, self.to_rgb, flip=True if self.flip else None)
        return dict(img=img, img_meta=self.meta(h, w))


class FrameIngestAug(object):
    """MultiScaleFlipAug(img_scale=[...], flip=...) around the same transforms (mmdet/datasets/pipelines/test_aug.py): one call per
    decoded frame -> dict(img=[A tensors [1, 3, pad_h, pad_w]], img_meta=[A metas]) in the reference's order -- scale outer, flip
    inner (un-flipped first).  The uint8 frame goes to the device once; every augmentation is one `hvr_ingest_frame(_flip)` launch.
    A video's frames ingested this way are what `VideoWindowRunner.step` and `forward_feat_aug` take: x[t][a], img_meta[t][a]."""

    def __init__(self, img_scale=((1000, 600),), flip=False, **kwargs):
        scales = [tuple(img_scale)] if isinstance(img_scale[0], (int, float)) else [tuple(s) for s in img_scale]
        flips = [False, True] if flip else [False]
        self.img_scale, self.flip = scales, bool(flip)
        self.ingests = [FrameIngest(img_scale=s, flip=f, **kwargs) for s in scales for f in flips]

    def metas(self, h, w):
        """The A metas of an h x w frame (host only)."""
        return [ing.meta(h, w) for ing in self.ingests]

    def __call__(self, frame):
        frame = self.ingests[0]._to_device(frame)
        outs = [ing(frame) for ing in self.ingests]
        return dict(img=[o['img'] for o in outs], img_meta=[o['img_meta'] for o in outs])
