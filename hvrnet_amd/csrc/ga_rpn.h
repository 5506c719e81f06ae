// Launch parameters of the guided proposal kernels (ga_rpn.hip), filled by the C ABI (capi.hip: hvr_ga_rpn_proposals).
#pragma once

namespace hvr {

struct GaParams {
  int T, H, W, npre, nms_pre, stride;
  int cls_pitch, reg_pitch, shape_pitch;
  float square[4];       // base square anchor at pixel (0, 0)
  float am[4], as[4];    // anchoring means / stds
  float tm[4], ts[4];    // target means / stds
  float a_ratio, t_ratio;  // |log(wh_ratio_clip)| of the anchoring step (1e-6) and of the proposal step (16 / 1000)
  float img_h, img_w;
};

}  // namespace hvr
