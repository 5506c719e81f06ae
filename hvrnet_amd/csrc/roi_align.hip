// RoIAlign forward / backward, legacy "+1 pixel" (non-aligned) convention.
// Replaces mmdet/ops/roi_align/src/roi_align_kernel.cu:16-141 (forward) and :143-282
// (backward).  Same arithmetic per sample point; different parallelisation:
//   * one workgroup per RoI, lanes along channels (NHWC: 16 B of channels per lane per
//     bilinear tap -> coalesced gathers, coalesced [roi][bin][C] stores),
//   * all frames of a window in ONE launch (the roi's batch index selects the frame),
//     where the reference launches once per frame (detectors/hnmb_rcnn.py:596-598).
// HBM-bound: bytes = feature map once + output once; taps hit L2.
// The tap rule (make_tap) and the RoI geometry (roi_geom) live in roi_align_dev.h, the per-bin bodies of the NHWC forward in the
// fragments roi_align_bins.h / roi_align_bins_s2.h: fpn.hip compiles the same statements behind a per-RoI level select.
#include "roi_align_dev.h"

namespace hvr {

// one axis of make_tap: the two cells a coordinate falls between and their weights (ok = false: outside (-1, size), no contribution)
struct AxisTap { int lo, hi; float wl, wh; bool ok; };
__device__ __forceinline__ AxisTap axis_tap(int size, float v) {
  AxisTap t;
  t.ok = !(v < -1.0f || v > (float)size);
  if (v <= 0.f) v = 0.f;
  int lo = (int)v, hi;
  if (lo >= size - 1) { hi = lo = size - 1; v = (float)lo; } else { hi = lo + 1; }
  if (!t.ok) { lo = hi = 0; v = 0.f; }
  const float l = v - lo;
  t.lo = lo; t.hi = hi; t.wl = 1.f - l; t.wh = l;
  return t;
}

// layout 1: features [B][H][W][C], output [K][PH][PW][C]; CV channels per lane
template <typename T, int CV>
__global__ __launch_bounds__(256) void roi_align_fwd_nhwc(const T* __restrict__ feat, const float* __restrict__ rois,
                                                          T* __restrict__ out, int C, int H, int W, int PH, int PW,
                                                          float spatial_scale, int sample_num) {
  const int k = blockIdx.x;
  const float* roi = rois + (long)k * 5;
#include "roi_align_bins.h"
}

// sample_num = 2, 2-byte elements, 16 B of channels per lane: the pipelined body (roi_align_bins_s2.h)
template <typename T>   // bf16_t / f16_t
__global__ __launch_bounds__(256) void roi_align_fwd_nhwc_bf16_s2(const T* __restrict__ feat, const float* __restrict__ rois,
                                                                  T* __restrict__ out, int C, int H, int W, int PH, int PW,
                                                                  float spatial_scale) {
  const int k = blockIdx.x;
  const float* roi = rois + (long)k * 5;
#include "roi_align_bins_s2.h"
}

// layout 0: features [B][C][H][W], output [K][C][PH][PW] -- the reference's own layout
// (kept for drop-in callers that hand NCHW tensors; one thread per output element).
template <typename T>
__global__ void roi_align_fwd_nchw(const T* __restrict__ feat, const float* __restrict__ rois, T* __restrict__ out,
                                   long total, int C, int H, int W, int PH, int PW, float spatial_scale, int sample_num) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total; index += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(index % PW), ph = (int)((index / PW) % PH);
    const int c = (int)((index / PW / PH) % C), n = (int)(index / PW / PH / C);
    const RoiGeom g = roi_geom(rois + (long)n * 5, spatial_scale, sample_num, PH, PW);
    const T* fb = feat + ((long)g.batch * C + c) * H * W;
    float acc = 0.f;
    for (int iy = 0; iy < g.sn_h; ++iy) {
      const float y = g.start_h + ph * g.bin_h + (iy + .5f) * g.bin_h / (float)g.sn_h;
      for (int ix = 0; ix < g.sn_w; ++ix) {
        const float x = g.start_w + pw * g.bin_w + (ix + .5f) * g.bin_w / (float)g.sn_w;
        const BilinearTap t = make_tap(H, W, y, x);
        if (!t.inside) continue;
        const float lt = ElemTraits<T>::load(fb + t.y_low * W + t.x_low), rt = ElemTraits<T>::load(fb + t.y_low * W + t.x_high);
        const float lb = ElemTraits<T>::load(fb + t.y_high * W + t.x_low), rb = ElemTraits<T>::load(fb + t.y_high * W + t.x_high);
        acc += (t.w1 * lt + t.w2 * rt + t.w3 * lb + t.w4 * rb);
      }
    }
    acc /= (float)(g.sn_h * g.sn_w);
    ElemTraits<T>::store(out + index, acc);
  }
}

// backward (f32 only, like the reference: roi_align_kernel.cu:269-272 rejects double and
// the training path runs f32): scatter grad * w / count with atomics.
// layout 1: grad_out [K][PH][PW][C] -> grad_in [B][H][W][C]; layout 0: NCHW both.
__global__ void roi_align_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ rois,
                                     float* __restrict__ gin, long total, int C, int H, int W, int PH, int PW,
                                     float spatial_scale, int sample_num, int nhwc) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total; index += (long)gridDim.x * blockDim.x) {
    int pw, ph, c, n;
    if (nhwc) {
      c = (int)(index % C); pw = (int)((index / C) % PW); ph = (int)((index / C / PW) % PH); n = (int)(index / C / PW / PH);
    } else {
      pw = (int)(index % PW); ph = (int)((index / PW) % PH); c = (int)((index / PW / PH) % C); n = (int)(index / PW / PH / C);
    }
    const RoiGeom g = roi_geom(rois + (long)n * 5, spatial_scale, sample_num, PH, PW);
    const float go = gout[index];
    const float count = (float)(g.sn_h * g.sn_w);
    if (nhwc && g.sn_h == 2 && g.sn_w == 2) {
      // 2 x 2 samples per bin (both configs), NHWC: the bilinear weights are separable, and the two sample rows (columns) of a bin mostly
      // fall into the same or adjacent feature rows -- their taps are merged per axis first, so a bin costs rows x cols = 4 .. 9 atomics
      // instead of 16 (round 6: the scatter is 0.6 - 0.9 ms of a training iteration).  Same sums, associated per axis.
      int ry[4], rx[4];
      float wy[4], wx[4];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const AxisTap ty = axis_tap(H, g.start_h + ph * g.bin_h + (s + .5f) * g.bin_h * .5f);
        const AxisTap tx = axis_tap(W, g.start_w + pw * g.bin_w + (s + .5f) * g.bin_w * .5f);
        ry[2 * s] = ty.lo; ry[2 * s + 1] = ty.hi; wy[2 * s] = ty.ok ? ty.wl : 0.f; wy[2 * s + 1] = ty.ok ? ty.wh : 0.f;
        rx[2 * s] = tx.lo; rx[2 * s + 1] = tx.hi; wx[2 * s] = tx.ok ? tx.wl : 0.f; wx[2 * s + 1] = tx.ok ? tx.wh : 0.f;
      }
#pragma unroll
      for (int j = 1; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < j; ++i) {
          if (ry[j] == ry[i] && wy[j] != 0.f) { wy[i] += wy[j]; wy[j] = 0.f; }
          if (rx[j] == rx[i] && wx[j] != 0.f) { wx[i] += wx[j]; wx[j] = 0.f; }
        }
      float* base = gin + (long)g.batch * H * W * C + c;
      const float gs = go / count;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (wy[a] == 0.f) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (wx[b] != 0.f) atomicAdd(base + ((long)ry[a] * W + rx[b]) * C, gs * wy[a] * wx[b]);
      }
      continue;
    }
    for (int iy = 0; iy < g.sn_h; ++iy) {
      const float y = g.start_h + ph * g.bin_h + (iy + .5f) * g.bin_h / (float)g.sn_h;
      for (int ix = 0; ix < g.sn_w; ++ix) {
        const float x = g.start_w + pw * g.bin_w + (ix + .5f) * g.bin_w / (float)g.sn_w;
        const BilinearTap t = make_tap(H, W, y, x);
        if (!t.inside) continue;
        const float g1 = go * t.w1 / count, g2 = go * t.w2 / count, g3 = go * t.w3 / count, g4 = go * t.w4 / count;
        if (nhwc) {
          float* base = gin + (long)g.batch * H * W * C + c;
          atomicAdd(base + ((long)t.y_low * W + t.x_low) * C, g1);
          atomicAdd(base + ((long)t.y_low * W + t.x_high) * C, g2);
          atomicAdd(base + ((long)t.y_high * W + t.x_low) * C, g3);
          atomicAdd(base + ((long)t.y_high * W + t.x_high) * C, g4);
        } else {
          float* base = gin + ((long)g.batch * C + c) * H * W;
          atomicAdd(base + t.y_low * W + t.x_low, g1);
          atomicAdd(base + t.y_low * W + t.x_high, g2);
          atomicAdd(base + t.y_high * W + t.x_low, g3);
          atomicAdd(base + t.y_high * W + t.x_high, g4);
        }
      }
    }
  }
}

template <typename T>
static hipError_t launch_roi_align_nhwc_h16(const void* feat, const float* rois, void* out, int C, int H, int W, int K, int PH, int PW, float scale,
                                            int sample_num, hipStream_t s) {
  const bool al16 = ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int form = roi_align_h16_form(C, sample_num, al16);
  if (form == ROI_FORM_S2) {
    hipLaunchKernelGGL(roi_align_fwd_nhwc_bf16_s2<T>, dim3(K), dim3(256), 0, s, (const T*)feat, rois, (T*)out, C, H, W, PH, PW, scale);
  } else if (form == ROI_FORM_CV8) {
    hipLaunchKernelGGL((roi_align_fwd_nhwc<T, 8>), dim3(K), dim3(256), 0, s, (const T*)feat, rois, (T*)out, C, H, W, PH, PW, scale, sample_num);
  } else if (form == ROI_FORM_CV4) {
    hipLaunchKernelGGL((roi_align_fwd_nhwc<T, 4>), dim3(K), dim3(256), 0, s, (const T*)feat, rois, (T*)out, C, H, W, PH, PW, scale, sample_num);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t run_roi_align_fwd(const void* feat, const float* rois, void* out, int B, int C, int H, int W, int K, int PH,
                             int PW, float scale, int sample_num, int dtype, int layout, hipStream_t s) {
  (void)B;
  if (K == 0) return hipSuccess;
  if (dtype == DT_F16S) return hipErrorInvalidValue;   // (split-half callers interpolate in f32 and cast)
  if (layout == 1) {
    if (dtype == DT_BF16) return launch_roi_align_nhwc_h16<bf16_t>(feat, rois, out, C, H, W, K, PH, PW, scale, sample_num, s);
    if (dtype == DT_F16) return launch_roi_align_nhwc_h16<f16_t>(feat, rois, out, C, H, W, K, PH, PW, scale, sample_num, s);
    if (!roi_align_f32_form(C)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((roi_align_fwd_nhwc<float, 4>), dim3(K), dim3(256), 0, s, (const float*)feat, rois, (float*)out, C, H, W, PH, PW, scale, sample_num);
  } else {
    const long total = (long)K * C * PH * PW;
    const int grid = (int)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    if (dtype == DT_BF16)
      hipLaunchKernelGGL(roi_align_fwd_nchw<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)feat, rois, (bf16_t*)out, total, C, H, W, PH, PW, scale, sample_num);
    else if (dtype == DT_F16)
      hipLaunchKernelGGL(roi_align_fwd_nchw<f16_t>, dim3(grid), dim3(256), 0, s, (const f16_t*)feat, rois, (f16_t*)out, total, C, H, W, PH, PW, scale, sample_num);
    else
      hipLaunchKernelGGL(roi_align_fwd_nchw<float>, dim3(grid), dim3(256), 0, s, (const float*)feat, rois, (float*)out, total, C, H, W, PH, PW, scale, sample_num);
  }
  return hipGetLastError();
}

hipError_t run_roi_align_bwd(const float* gout, const float* rois, float* gin, int C, int H, int W, int K, int PH, int PW,
                             float scale, int sample_num, int layout, hipStream_t s) {
  if (K == 0) return hipSuccess;
  const long total = (long)K * C * PH * PW;
  const int grid = (int)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  hipLaunchKernelGGL(roi_align_bwd_kernel, dim3(grid), dim3(256), 0, s, gout, rois, gin, total, C, H, W, PH, PW, scale, sample_num, layout);
  return hipGetLastError();
}

}  // namespace hvr
