// The smooth-L1 element of the RPN losses (losses/smooth_l1_loss.py:9-18), shared by rpn_loss_kernel (targets.hip) and
// rpn_focal_loss_kernel (focal.hip).  Both units are built with -ffp-contract=off, so the two kernels round alike.
#pragma once
#include <hip/hip_runtime.h>

namespace hvr {

// d = pred - target, bw the element's box weight, avg the kernel's avg_factor: returns the loss term smoothL1_beta(d) * bw (to be
// summed, then divided by avg) and sets *grad = bw / avg * d smoothL1 / d d.
__device__ __forceinline__ float smooth_l1_term(float d, float beta, float bw, float avg, float* grad) {
  const float ad = fabsf(d);
  *grad = bw / avg * (ad < beta ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)));
  return (ad < beta ? 0.5f * ad * ad / beta : ad - 0.5f * beta) * bw;
}

}  // namespace hvr
