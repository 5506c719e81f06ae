"""hvrnet_amd -- MI355X-native HVRNet video-detection forward path.

Importing the package registers the hot-path components under the reference's names
(ResNet, ResNeXt, Res2Net, ResLayer, ResXLayer, Res2Layer, FPN, RPNHead, GARPNHead, SingleRoIExtractor, SelsaBBoxHead, HRNMPBBoxHead, SelsaRCNN, HNMBRCNN).
"""
__version__ = '0.1.0'

from . import registry  # noqa: F401
from .backbone import (Bottle2neck, Res2Layer, Res2Net, ResLayer, ResNet, ResNeXt, ResXLayer, enable_training, make_res2_layer,  # noqa: F401
                       set_compute_dtype)
from .bbox_heads import BBoxHead, HRNMPBBoxHead, SelsaBBoxHead  # noqa: F401
from .box_ops import (bbox_flip, bbox_mapping, bbox_mapping_back, merge_aug_bboxes, merge_aug_proposals,  # noqa: F401
                      merge_aug_scores)
from .config import Config, hvr_config, selsa_config  # noqa: F401
from .detectors import HNMBRCNN, SelsaRCNN  # noqa: F401
from .ga_rpn_head import GARPNHead  # noqa: F401
from . import losses  # noqa: F401
from .losses import (FocalLoss, SmoothL1Loss, BalancedL1Loss, MSELoss, IoULoss, BoundedIoULoss, GHMC, GHMR)  # noqa: F401
from .necks import FPN  # noqa: F401
from .ops import ContextBlock, GeneralizedAttention, MaskedConv2d, RoIPool, masked_conv2d, roi_pool, seq_nms, soft_nms  # noqa: F401
from .pipelines import FrameIngest, FrameIngestAug  # noqa: F401
from .registry import build_detector, build_neck  # noqa: F401
from .roi_extractor import SingleRoIExtractor  # noqa: F401
from .rpn_head import RPNHead  # noqa: F401


def build_model(cfg, state_dict=None, dtype=None, device='cuda:0'):
    """Detector from a Config (reference file or built-in), optionally loading a reference-keyed state dict."""
    import torch
    model = build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    if state_dict is not None:
        model.load_state_dict(state_dict, strict=True)
    model.eval()
    if dtype is not None:
        set_compute_dtype(model, dtype)
    if device is not None and torch.cuda.is_available():
        model.to(device)
    return model
