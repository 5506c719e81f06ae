// The multi-level feature path: the FPN top-down merge and RoIAlign over up to four maps, one launch each.  The rules are stated in
// include/hvr_hip.h (hvr_fpn_merge, hvr_roi_align_levels_fwd).
//   * fpn_merge_kernel: replaces the L - 1 `laterals[i - 1] += F.interpolate(laterals[i], scale_factor=2, mode='nearest')` steps
//     of mmdet/models/necks/fpn.py:117-120.  One lane per 16-byte piece of an output pixel, every level below the top in the same
//     launch; a lane sums its pixel's chain of laterals in f32 from the coarsest level inwards and rounds once.  A level reads
//     laterals only, never another level's output: workgroups need no order.  HBM-bound: every lateral read once (the coarse
//     re-reads hit L2), every output written once.
//   * roi_align_levels_kernel: replaces the per-level loop of mmdet/models/roi_extractors/single_level.py:89-107 (map_roi_levels,
//     the `inds.any()` host read per level, gather / pool / scatter into a zeroed output).  One workgroup per RoI, as roi_align.hip;
//     the workgroup computes its RoI's level, takes that level's map, size and scale, and runs the bins through the body fragments
//     roi_align_bins.h / roi_align_bins_s2.h -- the statements roi_align.hip compiles.  A level without RoIs has no workgroup.
#include "roi_align_dev.h"

namespace hvr {

constexpr int kFpnMaxLevels = 4;

struct FpnMergeParams {
  const void* lat[kFpnMaxLevels];
  void* out[kFpnMaxLevels];     // out[L - 1] unused
  long start[kFpnMaxLevels];    // first piece of level l in the flat index; start[L - 1] = total
  int H[kFpnMaxLevels], W[kFpnMaxLevels];
  int L, pieces;                // pieces = C / CV, 16-byte pieces per pixel
};

template <typename T> struct FpnVec { static constexpr int CV = 8; };
template <> struct FpnVec<float> { static constexpr int CV = 4; };

template <typename T> __device__ __forceinline__ void fpn_load(const T* p, float* f) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  } else {
    unpack2<T>(r.x, f[0], f[1]); unpack2<T>(r.y, f[2], f[3]); unpack2<T>(r.z, f[4], f[5]); unpack2<T>(r.w, f[6], f[7]);
  }
}
template <typename T> __device__ __forceinline__ void fpn_store(T* p, const float* f) {
  if constexpr (std::is_same<T, float>::value)
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  else
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}

// out[l](b, h, w) = lat[l](b, h, w) + m[l + 1](b, h >> 1, w >> 1), m[j] = lat[j] + m[j + 1](>> 1), m[L - 1] = lat[L - 1]: the chain
// of the pixel's ancestors, summed from the top down.  JUMP levels above l are read; the loop is unrolled per instance of JUMP so
// that the loads of a chain are issued together (they do not depend on each other).
template <typename T, int JUMP>
__device__ __forceinline__ void fpn_merge_piece(const FpnMergeParams& p, int l, long pix, int piece) {
  constexpr int CV = FpnVec<T>::CV;
  const int H = p.H[l], W = p.W[l];
  const int w = (int)(pix % W);
  const long bh = pix / W;
  const int h = (int)(bh % H);
  const long b = bh / H;
  const long C = (long)p.pieces * CV;
  float v[JUMP + 1][CV];
  fpn_load<T>((const T*)p.lat[l] + pix * C + (long)piece * CV, v[0]);
#pragma unroll
  for (int j = 1; j <= JUMP; ++j) {
    const long src = (b * p.H[l + j] + (h >> j)) * p.W[l + j] + (w >> j);
    fpn_load<T>((const T*)p.lat[l + j] + src * C + (long)piece * CV, v[j]);
  }
  float acc[CV];
#pragma unroll
  for (int e = 0; e < CV; ++e) acc[e] = v[JUMP][e];
#pragma unroll
  for (int j = JUMP - 1; j >= 0; --j)
#pragma unroll
    for (int e = 0; e < CV; ++e) acc[e] = v[j][e] + acc[e];
  fpn_store<T>((T*)p.out[l] + pix * C + (long)piece * CV, acc);
}

template <typename T>
__global__ __launch_bounds__(256) void fpn_merge_kernel(const FpnMergeParams p) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int L = p.L;
  if (idx >= p.start[L - 1]) return;
  int l = 0;
  if (L > 2 && idx >= p.start[1]) l = 1;
  if (L > 3 && idx >= p.start[2]) l = 2;
  const long rel = idx - p.start[l];
  const long pix = rel / p.pieces;
  const int piece = (int)(rel - pix * p.pieces);
  switch (L - 1 - l) {
    case 1: fpn_merge_piece<T, 1>(p, l, pix, piece); break;
    case 2: fpn_merge_piece<T, 2>(p, l, pix, piece); break;
    default: fpn_merge_piece<T, 3>(p, l, pix, piece); break;
  }
}

// shapes, the instance set, alignment and aliasing are validated by the C ABI (capi.hip: hvr_fpn_merge)
hipError_t run_fpn_merge(const void* const* lat, void* const* out, int L, int B, const int* H, const int* W, int C, int dtype, hipStream_t s) {
  if (L <= 1) return hipSuccess;   // the top level's merged map is its lateral
  FpnMergeParams p;
  const int cv = dtype == DT_F32 ? 4 : 8;
  p.L = L;
  p.pieces = C / cv;
  long total = 0;
  for (int l = 0; l < kFpnMaxLevels; ++l) {
    p.lat[l] = l < L ? lat[l] : nullptr;
    p.out[l] = l < L - 1 ? out[l] : nullptr;
    p.H[l] = l < L ? H[l] : 1;
    p.W[l] = l < L ? W[l] : 1;
    p.start[l] = total;
    if (l < L - 1) total += (long)B * H[l] * W[l] * p.pieces;
  }
  if (total == 0) return hipSuccess;
  const long grid = (total + 255) / 256;
  if (grid > 0x7fffffffL) return hipErrorInvalidValue;
  if (dtype == DT_BF16) hipLaunchKernelGGL(fpn_merge_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, s, p);
  else if (dtype == DT_F16) hipLaunchKernelGGL(fpn_merge_kernel<f16_t>, dim3((unsigned)grid), dim3(256), 0, s, p);
  else if (dtype == DT_F32) hipLaunchKernelGGL(fpn_merge_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- RoIAlign over several levels ----
struct RoiLevelsParams {
  const void* feat[kFpnMaxLevels];
  int H[kFpnMaxLevels], W[kFpnMaxLevels];
  float scale[kFpnMaxLevels];
  int L, C, PH, PW, sample_num;
  float finest_scale;
  const float* rois;        // [K][5]: decide the level
  const float* pool_rois;   // [K][5]: pooled
  void* out;                // [K][PH][PW][C]
  int* levels;              // [K] or null
};

// The level of a RoI (single_level.py:55-73, map_roi_levels): floor(log2(sqrt(w * h) / finest_scale + 1e-6)) clamped to [0, L - 1],
// as comparisons with the powers of two.  f32, every operation rounded on its own: the pragma keeps contraction out, the division
// and the square root are the correctly rounded ones (sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that name is
// the native approximation).  A NaN (exactly one side negative) fails every comparison: level 0.
__device__ __forceinline__ int roi_level(const float* roi, float finest_scale, int L) {
#pragma clang fp contract(off)
  const float w = __fadd_rn(__fsub_rn(roi[3], roi[1]), 1.f);
  const float h = __fadd_rn(__fsub_rn(roi[4], roi[2]), 1.f);
  const float s = sqrtf(__fmul_rn(w, h));
  const float v = __fadd_rn(__fdiv_rn(s, finest_scale), 1e-6f);
  int level = 0;
  if (L > 1 && v >= 2.f) ++level;
  if (L > 2 && v >= 4.f) ++level;
  if (L > 3 && v >= 8.f) ++level;
  return level;
}

// FORM: the body fragment the single-map call runs at this C (ROI_FORM_*; f32 maps: ROI_FORM_CV4)
template <typename T, int FORM>
__global__ __launch_bounds__(256) void roi_align_levels_kernel(const RoiLevelsParams p) {
  const int k = blockIdx.x;
  // every lane computes the same level; readfirstlane says so to the compiler: the map, its size and its scale stay scalar
  const int lvl = __builtin_amdgcn_readfirstlane(roi_level(p.rois + (long)k * 5, p.finest_scale, p.L));
  if (threadIdx.x == 0 && p.levels) p.levels[k] = lvl;
  const void* map = p.feat[0];
  int H = p.H[0], W = p.W[0];
  float spatial_scale = p.scale[0];
  if (lvl == 1) { map = p.feat[1]; H = p.H[1]; W = p.W[1]; spatial_scale = p.scale[1]; }
  if (lvl == 2) { map = p.feat[2]; H = p.H[2]; W = p.W[2]; spatial_scale = p.scale[2]; }
  if (lvl == 3) { map = p.feat[3]; H = p.H[3]; W = p.W[3]; spatial_scale = p.scale[3]; }
  // what the body fragments expect in scope
  const T* __restrict__ feat = (const T*)map;
  const float* __restrict__ roi = p.pool_rois + (long)k * 5;
  T* __restrict__ out = (T*)p.out;
  const int C = p.C, PH = p.PH, PW = p.PW;
  if constexpr (FORM == ROI_FORM_S2) {
#include "roi_align_bins_s2.h"
  } else if constexpr (FORM == ROI_FORM_CV8) {
    constexpr int CV = 8;
    const int sample_num = p.sample_num;
#include "roi_align_bins.h"
  } else {
    constexpr int CV = 4;
    const int sample_num = p.sample_num;
#include "roi_align_bins.h"
  }
}

template <typename T>
static hipError_t launch_roi_levels_h16(const RoiLevelsParams& p, int K, bool al16, hipStream_t s) {
  const int form = roi_align_h16_form(p.C, p.sample_num, al16);
  if (form == ROI_FORM_S2) hipLaunchKernelGGL((roi_align_levels_kernel<T, ROI_FORM_S2>), dim3(K), dim3(256), 0, s, p);
  else if (form == ROI_FORM_CV8) hipLaunchKernelGGL((roi_align_levels_kernel<T, ROI_FORM_CV8>), dim3(K), dim3(256), 0, s, p);
  else if (form == ROI_FORM_CV4) hipLaunchKernelGGL((roi_align_levels_kernel<T, ROI_FORM_CV4>), dim3(K), dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

int roi_align_levels_instance(int C, int dtype) {
  if (dtype == DT_F32) return roi_align_f32_form(C);
  if (dtype == DT_BF16 || dtype == DT_F16) return roi_align_h16_form(C, 0, false) != ROI_FORM_NONE;
  return 0;
}

hipError_t run_roi_align_levels(const void* const* feat, const int* H, const int* W, const float* scale, int L, int C, int K, int PH, int PW,
                                int sample_num, int dtype, float finest_scale, const float* rois, const float* pool_rois, void* out,
                                int* levels, hipStream_t s) {
  if (K == 0) return hipSuccess;
  RoiLevelsParams p;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out);
  for (int l = 0; l < kFpnMaxLevels; ++l) {
    const int i = l < L ? l : 0;   // unused slots repeat level 0
    p.feat[l] = feat[i]; p.H[l] = H[i]; p.W[l] = W[i]; p.scale[l] = scale[i];
    bits |= reinterpret_cast<uintptr_t>(feat[i]);
  }
  p.L = L; p.C = C; p.PH = PH; p.PW = PW; p.sample_num = sample_num;
  p.finest_scale = finest_scale;
  p.rois = rois; p.pool_rois = pool_rois; p.out = out; p.levels = levels;
  if (dtype == DT_BF16) return launch_roi_levels_h16<bf16_t>(p, K, (bits & 15) == 0, s);
  if (dtype == DT_F16) return launch_roi_levels_h16<f16_t>(p, K, (bits & 15) == 0, s);
  if (dtype != DT_F32 || !roi_align_f32_form(C)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((roi_align_levels_kernel<float, ROI_FORM_CV4>), dim3(K), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace hvr
