"""SingleRoIExtractor (mmdet/models/roi_extractors/single_level.py:11-107).

`roi_layer` is resolved by name from `hvrnet_amd.ops`, exactly as the reference resolves it from
`mmdet.ops` (single_level.py:45-52).  With one level the reference returns
`self.roi_layers[0](feats[0], rois)` (single_level.py:91-92), and so does this class (`featmap_strides=[16]` in both
window configs).  With several levels (the maps of an FPN neck) the reference maps every RoI to a level, loops over
the levels, reads `inds.any()` on the host in each pass, and gathers, pools and scatters into a zeroed output
(single_level.py:94-107); here that is ONE `native.roi_align_levels` call over the first `num_inputs` maps: no host
read, no zero fill (the level rule and where it differs from torch's `floor(log2())`: include/hvr_hip.h).  Several
levels take `RoIAlign` layers only; inference only.
"""
import torch.nn as nn

from . import native, ops
from .registry import ROI_EXTRACTORS


@ROI_EXTRACTORS.register_module
class SingleRoIExtractor(nn.Module):

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super(SingleRoIExtractor, self).__init__()
        self.roi_layers = self.build_roi_layers(roi_layer, featmap_strides)
        self.out_channels = out_channels
        self.featmap_strides = featmap_strides
        self.finest_scale = finest_scale
        self.fp16_enabled = False

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    def build_roi_layers(self, layer_cfg, featmap_strides):
        cfg = layer_cfg.copy()
        layer_type = cfg.pop('type')
        assert hasattr(ops, layer_type)
        layer_cls = getattr(ops, layer_type)
        return nn.ModuleList([layer_cls(spatial_scale=1 / s, **cfg) for s in featmap_strides])

    def forward(self, feats, rois, roi_scale_factor=None):
        if len(feats) == 1:
            return self.roi_layers[0](feats[0], rois)
        feats = feats[:self.num_inputs]
        layer = self.roi_layers[0]
        if not all(type(m) is ops.RoIAlign for m in self.roi_layers):
            raise NotImplementedError('roi_layer %s at %d levels is outside the HIP path: several levels take RoIAlign only'
                                      % (type(layer).__name__, len(feats)))
        if len(feats) > native.FPN_MAX_LEVELS:
            raise NotImplementedError('featmap_strides: %d levels, the multi-level RoIAlign kernel takes %d' % (len(feats), native.FPN_MAX_LEVELS))
        if not feats[0].is_cuda:
            raise NotImplementedError('SingleRoIExtractor runs on the GPU only (no CPU fallback)')
        maps = [ops._pooling_map(f) for f in feats]   # logical NCHW over physical NHWC: used in place
        out = native.roi_align_levels(maps, rois, layer.out_size, [m.spatial_scale for m in self.roi_layers[:len(maps)]],
                                      finest_scale=self.finest_scale, sample_num=layer.sample_num, roi_scale_factor=roi_scale_factor)
        return out.permute(0, 3, 1, 2)
