// RoI max pooling, forward (with or without the argmax) and the argmax backward.
// Replaces mmdet/ops/roi_pool/src/roi_pool_kernel.cu:16-74 (forward) and :112-135 (backward).  The rule -- the bin geometry in f32,
// the first-maximum selection, empty bins, malformed RoIs and batch indices outside the call -- is stated in include/hvr_hip.h;
// RoIAlign's layout and parallelisation (roi_align.hip), not the reference's one-thread-per-output flat index:
//   * one workgroup per RoI, all frames of a call in ONE launch (the roi's batch index selects the frame);
//   * the map is physical NHWC: lanes run along channels, 16 bytes of channels per lane, the bins are spread over the remaining
//     lane groups; stores are whole contiguous pieces of out / argmax [roi][bin][C];
//   * a lane walks its bin's pixels h-major with a running maximum (and, in the argmax form, a running index) under a strict `>`:
//     the first pixel that attains the maximum wins.  The loads do not depend on the data, so the walk pipelines.
// Values are compared after an exact widening to f32 and stored through the narrowing that inverts it: the stored result is the
// input element.  `v > m ? v : m`, not fmaxf: of +0 and -0 the FIRST stays, as the rule says.
// Built with -ffp-contract=off (build.sh): a bin edge is floor / ceil of a product plus a sum, each rounded on its own; a fused
// multiply-add moves edges that land on a pixel boundary (include/hvr_hip.h names three such RoIs).
#include "common.h"

namespace hvr {

template <typename T> struct RpVec { static constexpr int CV = 8; };
template <> struct RpVec<float> { static constexpr int CV = 4; };

template <typename T> __device__ __forceinline__ void rp_load(const T* p, float* f) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  } else {
    unpack2<T>(r.x, f[0], f[1]); unpack2<T>(r.y, f[2], f[3]); unpack2<T>(r.z, f[4], f[5]); unpack2<T>(r.w, f[6], f[7]);
  }
}
template <typename T> __device__ __forceinline__ void rp_store(T* p, const float* f) {
  if constexpr (std::is_same<T, float>::value)
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  else   // (every f is a widened T: the narrowing is exact)
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}

// one bin edge: clamped into [0, size] as a float, then converted (any finite or infinite coordinate is safe; NaN gives 0)
__device__ __forceinline__ int rp_edge(float v, int size) { return (int)fminf(fmaxf(v, 0.f), (float)size); }

template <typename T, bool ARG>
__global__ __launch_bounds__(256) void roi_pool_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ rois, T* __restrict__ out,
                                                           int32_t* __restrict__ argmax, int B, int H, int W, int C, int PH, int PW, float scale) {
  constexpr int CV = RpVec<T>::CV;
  const int k = blockIdx.x;
  const int lanes_c = C / CV;                            // 16-byte pieces of one output bin
  const int lanes_used = lanes_c < 256 ? lanes_c : 256;  // threads along channels
  const int groups = 256 / lanes_used;                   // bins in flight
  const int grp = (int)threadIdx.x / lanes_used, cl0 = (int)threadIdx.x - grp * lanes_used;
  if (grp >= groups) return;
  const float* roi = rois + (long)k * 5;
  const float bf = roi[0];
  const bool frame_ok = bf >= 0.f && bf < (float)B;      // (NaN: false)
  const int b = frame_ok ? (int)bf : 0;
  const float rx1 = roi[1] * scale, ry1 = roi[2] * scale;
  const float rx2 = (roi[3] + 1.f) * scale, ry2 = (roi[4] + 1.f) * scale;
  const float rw = rx2 - rx1, rh = ry2 - ry1;
  const bool roi_ok = frame_ok && rw > 0.f && rh > 0.f;  // malformed, or a frame outside the call: nothing is read
  const float bw = rw / (float)PW, bh = rh / (float)PH;
  const T* fb = feat + (long)b * H * W * C;
  for (int bin = grp; bin < PH * PW; bin += groups) {
    const int ph = bin / PW, pw = bin - ph * PW;
    const int xs = rp_edge(floorf((float)pw * bw + rx1), W), xe = rp_edge(ceilf((float)(pw + 1) * bw + rx1), W);
    const int ys = rp_edge(floorf((float)ph * bh + ry1), H), ye = rp_edge(ceilf((float)(ph + 1) * bh + ry1), H);
    const bool empty = !roi_ok || xe <= xs || ye <= ys;
    for (int cl = cl0; cl < lanes_c; cl += lanes_used) {
      const long o = ((long)k * PH * PW + bin) * C + (long)cl * CV;
      float m[CV];
      int idx[CV];
      if (empty) {
#pragma unroll
        for (int e = 0; e < CV; ++e) { m[e] = 0.f; idx[e] = -1; }
      } else {
        const T* fc = fb + (long)cl * CV;
        rp_load<T>(fc + ((long)ys * W + xs) * C, m);     // the bin's first pixel; the walk below meets it again and `>` passes it by
#pragma unroll
        for (int e = 0; e < CV; ++e) idx[e] = ys * W + xs;
        for (int h = ys; h < ye; ++h) {
          const T* fr = fc + (long)h * W * C;
#pragma unroll 4
          for (int w = xs; w < xe; ++w) {
            float v[CV];
            rp_load<T>(fr + (long)w * C, v);
#pragma unroll
            for (int e = 0; e < CV; ++e) {
              const bool gt = v[e] > m[e];
              m[e] = gt ? v[e] : m[e];
              if constexpr (ARG) idx[e] = gt ? h * W + w : idx[e];
            }
          }
        }
      }
      rp_store<T>(out + o, m);
      if constexpr (ARG) {
#pragma unroll
        for (int e = 0; e < CV; e += 4) *reinterpret_cast<int4*>(argmax + o + e) = make_int4(idx[e], idx[e + 1], idx[e + 2], idx[e + 3]);
      }
    }
  }
}

// grad_feat[b][argmax][c] += grad_out[k][ph][pw][c] for argmax >= 0: one lane per output element, channels fastest, so neighbouring
// lanes hit neighbouring addresses.  A batch index outside [0, B) or an argmax outside the plane adds nothing (the forward never
// records one; the guard keeps a foreign argmax tensor from writing outside grad_feat).
__global__ __launch_bounds__(256) void roi_pool_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ rois,
                                                           const int32_t* __restrict__ argmax, float* __restrict__ gin, long total, int B,
                                                           int HW, int C, int bins) {
  for (long index = (long)blockIdx.x * blockDim.x + threadIdx.x; index < total; index += (long)gridDim.x * blockDim.x) {
    const int a = argmax[index];
    if (a < 0 || a >= HW) continue;
    const int c = (int)(index % C);
    const long k = index / C / bins;
    const float bf = rois[k * 5];
    if (!(bf >= 0.f && bf < (float)B)) continue;
    atomicAdd(gin + ((long)(int)bf * HW + a) * C + c, gout[index]);
  }
}

template <typename T>
static hipError_t launch_roi_pool_fwd(const void* feat, const float* rois, void* out, int32_t* argmax, int B, int H, int W, int C, int K, int PH,
                                      int PW, float scale, hipStream_t s) {
  if (argmax)
    hipLaunchKernelGGL((roi_pool_fwd_kernel<T, true>), dim3(K), dim3(256), 0, s, (const T*)feat, rois, (T*)out, argmax, B, H, W, C, PH, PW, scale);
  else
    hipLaunchKernelGGL((roi_pool_fwd_kernel<T, false>), dim3(K), dim3(256), 0, s, (const T*)feat, rois, (T*)out, argmax, B, H, W, C, PH, PW, scale);
  return hipGetLastError();
}

// shapes, the channel multiple and the alignment are validated by the C ABI (capi.hip: hvr_roi_pool_fwd / hvr_roi_pool_bwd)
hipError_t run_roi_pool_fwd(const void* feat, const float* rois, void* out, int32_t* argmax, int B, int H, int W, int C, int K, int PH, int PW,
                            float scale, int dtype, hipStream_t s) {
  if (K == 0) return hipSuccess;
  if (dtype == DT_BF16) return launch_roi_pool_fwd<bf16_t>(feat, rois, out, argmax, B, H, W, C, K, PH, PW, scale, s);
  if (dtype == DT_F16) return launch_roi_pool_fwd<f16_t>(feat, rois, out, argmax, B, H, W, C, K, PH, PW, scale, s);
  if (dtype == DT_F32) return launch_roi_pool_fwd<float>(feat, rois, out, argmax, B, H, W, C, K, PH, PW, scale, s);
  return hipErrorInvalidValue;
}

hipError_t run_roi_pool_bwd(const float* gout, const float* rois, const int32_t* argmax, float* gin, int B, int H, int W, int C, int K, int PH,
                            int PW, hipStream_t s) {
  if (K == 0) return hipSuccess;
  const long total = (long)K * PH * PW * C;
  const int grid = (int)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  hipLaunchKernelGGL(roi_pool_bwd_kernel, dim3(grid), dim3(256), 0, s, gout, rois, argmax, gin, total, B, H * W, C, PH * PW);
  return hipGetLastError();
}

}  // namespace hvr
