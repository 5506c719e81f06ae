// RoIAlign's device arithmetic, shared by roi_align.hip (one map per launch) and fpn.hip (up to four maps behind a per-RoI level
// select): the tap rule, the RoI geometry and which per-bin body a shape takes.  The bodies themselves are the fragments
// roi_align_bins.h / roi_align_bins_s2.h, which both units include inside their kernels, so a RoI pooled on its level gives the bits of
// the single-map call on that level's map.
#pragma once
#include "common.h"

namespace hvr {

struct BilinearTap {
  int y_low, x_low, y_high, x_high;
  float w1, w2, w3, w4;  // all zero when the point is outside (-1, H) x (-1, W)
  bool inside;
};

// roi_align_kernel.cu:16-61 (value) / :143-183 (gradient weights): identical index rule
__device__ __forceinline__ BilinearTap make_tap(int height, int width, float y, float x) {
  BilinearTap t;
  if (y < -1.0f || y > (float)height || x < -1.0f || x > (float)width) {
    t.y_low = t.x_low = t.y_high = t.x_high = 0;
    t.w1 = t.w2 = t.w3 = t.w4 = 0.f;
    t.inside = false;
    return t;
  }
  if (y <= 0.f) y = 0.f;
  if (x <= 0.f) x = 0.f;
  int y_low = (int)y, x_low = (int)x, y_high, x_high;
  if (y_low >= height - 1) { y_high = y_low = height - 1; y = (float)y_low; } else { y_high = y_low + 1; }
  if (x_low >= width - 1) { x_high = x_low = width - 1; x = (float)x_low; } else { x_high = x_low + 1; }
  const float ly = y - y_low, lx = x - x_low, hy = 1.f - ly, hx = 1.f - lx;
  t.y_low = y_low; t.x_low = x_low; t.y_high = y_high; t.x_high = x_high;
  t.w1 = hy * hx; t.w2 = hy * lx; t.w3 = ly * hx; t.w4 = ly * lx;
  t.inside = true;
  return t;
}

struct RoiGeom {
  int batch;
  float start_w, start_h, bin_w, bin_h;
  int sn_h, sn_w;
};

// roi_align_kernel.cu:76-99
__device__ __forceinline__ RoiGeom roi_geom(const float* roi, float spatial_scale, int sample_num, int ph, int pw) {
  RoiGeom g;
  g.batch = (int)roi[0];
  g.start_w = roi[1] * spatial_scale;
  g.start_h = roi[2] * spatial_scale;
  const float end_w = (roi[3] + 1.f) * spatial_scale, end_h = (roi[4] + 1.f) * spatial_scale;
  const float roi_w = fmaxf(end_w - g.start_w, 0.f), roi_h = fmaxf(end_h - g.start_h, 0.f);
  g.bin_h = roi_h / ph;
  g.bin_w = roi_w / pw;
  g.sn_h = sample_num > 0 ? sample_num : (int)ceilf(roi_h / ph);
  g.sn_w = sample_num > 0 ? sample_num : (int)ceilf(roi_w / pw);
  return g;
}

// the 16-byte pieces of the pipelined body (roi_align_bins_s2.h)
template <typename T> __device__ __forceinline__ void unpack8(const uint4& v, float f[8]) {
  unpack2<T>(v.x, f[0], f[1]); unpack2<T>(v.y, f[2], f[3]); unpack2<T>(v.z, f[4], f[5]); unpack2<T>(v.w, f[6], f[7]);
}

// Which body a 2-byte NHWC forward of C channels runs (256 lanes per workgroup): both units ask here, so a level pooled by fpn.hip
// takes the body the single-map call takes.  al16: every map and the output 16-byte aligned.
enum { ROI_FORM_NONE = 0, ROI_FORM_S2 = 1, ROI_FORM_CV8 = 2, ROI_FORM_CV4 = 3 };
inline int roi_align_h16_form(int C, int sample_num, bool al16) {
  const bool cv8 = C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0;
  if (cv8 && sample_num == 2 && al16) return ROI_FORM_S2;
  if (cv8) return ROI_FORM_CV8;
  if (C % 4 == 0 && C / 4 <= 256) return ROI_FORM_CV4;
  return ROI_FORM_NONE;
}
inline bool roi_align_f32_form(int C) { return C % 4 == 0 && C / 4 <= 256; }

}  // namespace hvr
