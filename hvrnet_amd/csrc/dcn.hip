// Deformable im2col (DCN v1 / v2 sampler), forward only.
// Replaces mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu:63-114 (bilinear rule), :190-242 (deformable_im2col_gpu_kernel) and
// :570-640 (modulated_deformable_im2col_gpu_kernel).  Same arithmetic per sample; a different layout and parallelisation:
//   * x is physical NHWC, so a bilinear corner is ONE contiguous channel vector: a lane owns 16 bytes of channels of one
//     (pixel, tap), resolves that tap's position, corner validities and weights once for all of them, issues its four corner
//     loads back to back (clamped addresses, always in bounds; a corner outside the map is zeroed after the load) and stores
//     16 bytes of the patch row.  Lanes run along [tap][channel], i.e. along the patch row: a wave's stores are whole
//     contiguous pieces of col, which is written exactly once.
//   * col [B*OH*OW][KH*KW*Cin] has the K order [kh][kw][cin] of the packed conv weights ([Cout][KH][KW][Cin]): the deformable
//     conv is the unchanged GEMM on it.
//   * offsets / mask logits come pixel-major ([B][OH][OW][ldo] f32, the raw output of the offset conv): the lanes of one
//     (pixel, tap, group) read the same two or three words (one broadcast fetch).
// Split half: the kernel reads and writes the [32 hi | 32 lo] container itself (merge2 is exact in f32; one split2 per output).
// Built with -ffp-contract=off (build.sh): every product and sum below is rounded on its own, which is what the f64 statement
// of the tests counts (tests/dcn_refs.py).  The mask is 1 / (1 + expf(-logit)) with the documented-accuracy expf and a
// correctly rounded add and divide -- no fast intrinsic.
#include "common.h"

namespace hvr {

template <typename T> struct DcnVec;   // channels per lane (16 bytes of the stored format; split half: 16 bytes of each plane)
template <> struct DcnVec<float> { static constexpr int kCV = 4; };
template <> struct DcnVec<bf16_t> { static constexpr int kCV = 8; };
template <> struct DcnVec<f16_t> { static constexpr int kCV = 8; };
template <> struct DcnVec<f16s_t> { static constexpr int kCV = 8; };

// the raw 16-byte pieces of one corner (split half: hi and lo plane)
template <typename T> struct DcnRaw { uint4 a; };
template <> struct DcnRaw<f16s_t> { uint4 a, b; };

template <typename T> __device__ __forceinline__ DcnRaw<T> dcn_load(const char* p) {
  DcnRaw<T> r;
  r.a = *reinterpret_cast<const uint4*>(p);
  if constexpr (std::is_same<T, f16s_t>::value) r.b = *reinterpret_cast<const uint4*>(p + kSplitPlane);
  return r;
}
__device__ __forceinline__ uint4 dcn_sel(bool ok, const uint4& v) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}
template <typename T> __device__ __forceinline__ void dcn_unpack(const DcnRaw<T>& r, bool ok, float* f) {
  const uint4 a = dcn_sel(ok, r.a);   // a corner outside the map contributes a zero VALUE (not a zero weight: 0 * inf would be NaN)
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
  } else if constexpr (std::is_same<T, f16s_t>::value) {
    const uint4 b = dcn_sel(ok, r.b);
    merge2(a.x, b.x, f[0], f[1]); merge2(a.y, b.y, f[2], f[3]); merge2(a.z, b.z, f[4], f[5]); merge2(a.w, b.w, f[6], f[7]);
  } else {
    unpack2<T>(a.x, f[0], f[1]); unpack2<T>(a.y, f[2], f[3]); unpack2<T>(a.z, f[4], f[5]); unpack2<T>(a.w, f[6], f[7]);
  }
}
template <typename T> __device__ __forceinline__ void dcn_store(char* p, const float* f) {
  if constexpr (std::is_same<T, float>::value) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  } else if constexpr (std::is_same<T, f16s_t>::value) {
    uint4 h, l;
    split2(f[0], f[1], h.x, l.x); split2(f[2], f[3], h.y, l.y); split2(f[4], f[5], h.z, l.z); split2(f[6], f[7], h.w, l.w);
    *reinterpret_cast<uint4*>(p) = h;
    *reinterpret_cast<uint4*>(p + kSplitPlane) = l;
  } else {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
  }
}
// byte offset of logical element e of a row
template <typename T> __device__ __forceinline__ long dcn_col_bytes(long e) {
  if constexpr (std::is_same<T, f16s_t>::value) return split_col_bytes(e);
  else if constexpr (std::is_same<T, float>::value) return e * 4;
  else return e * 2;
}

// one axis of deform_conv_cuda_kernel.cu:88-108: the two cells (clamped into the map for the load), whether each lies inside
// the map, and the two weights.  v is inside (-1, size) whenever the result is used.
struct DcnAxis { int lo, hi; bool lo_ok, hi_ok; float wl, wh; };
__device__ __forceinline__ DcnAxis dcn_axis(int size, float v) {
  DcnAxis t;
  const float vc = fminf(fmaxf(v, -1.f), (float)size);   // (NaN -> -1: the sample is dropped by the caller's test, the address stays in bounds)
  const float fl = floorf(vc);
  const int lo = (int)fl, hi = lo + 1;
  t.lo_ok = lo >= 0 && lo <= size - 1;
  t.hi_ok = hi >= 0 && hi <= size - 1;
  t.lo = min(max(lo, 0), size - 1);
  t.hi = min(max(hi, 0), size - 1);
  t.wh = vc - fl;          // lh
  t.wl = 1.f - t.wh;       // hh
  return t;
}

template <typename T, bool MOD>
__global__ __launch_bounds__(256) void deform_im2col_kernel(const char* __restrict__ x, const float* __restrict__ om, char* __restrict__ col,
                                                            unsigned total, int M, int H, int W, int Cin, int OH, int OW, int KH, int KW,
                                                            int stride, int pad, int dil, int dg, long ldo) {
  constexpr int CV = DcnVec<T>::kCV;
  const unsigned LC = (unsigned)(Cin / CV);       // lanes of one (pixel, tap)
  const unsigned KK = (unsigned)(KH * KW);
  const int cpg = Cin / dg;                       // channels of one deformable group (a multiple of 8: a lane never straddles two)
  const long row_bytes = dcn_col_bytes<T>(Cin);   // one pixel of x; a patch row is KK of them
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const unsigned u = idx / LC, cl = idx - u * LC;
    const unsigned m = u / KK, k = u - m * KK;    // output pixel (row of col), tap
    const int kh = (int)(k / (unsigned)KW), kw = (int)k - kh * KW;
    const int ox = (int)(m % (unsigned)OW), t = (int)(m / (unsigned)OW);
    const int oy = t % OH, b = t / OH;
    const int c0 = (int)cl * CV;
    const int g = c0 / cpg;
    const float* o = om + (long)m * ldo;
    const float off_h = o[g * 2 * (int)KK + 2 * (int)k], off_w = o[g * 2 * (int)KK + 2 * (int)k + 1];
    float mask = 1.f;
    if constexpr (MOD) {
      const float logit = o[2 * dg * (int)KK + g * (int)KK + (int)k];
      mask = 1.f / (1.f + expf(-logit));
    }
    // deform_conv_cuda_kernel.cu:226-227 / :614-615: the integer part in integer arithmetic, then ONE f32 add
    const float h = (float)(oy * stride - pad + kh * dil) + off_h;
    const float w = (float)(ox * stride - pad + kw * dil) + off_w;
    const bool inside = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
    const DcnAxis ay = dcn_axis(H, h), ax = dcn_axis(W, w);
    const char* xb = x + (long)b * H * W * row_bytes + dcn_col_bytes<T>(c0);
    const DcnRaw<T> r1 = dcn_load<T>(xb + ((long)ay.lo * W + ax.lo) * row_bytes);
    const DcnRaw<T> r2 = dcn_load<T>(xb + ((long)ay.lo * W + ax.hi) * row_bytes);
    const DcnRaw<T> r3 = dcn_load<T>(xb + ((long)ay.hi * W + ax.lo) * row_bytes);
    const DcnRaw<T> r4 = dcn_load<T>(xb + ((long)ay.hi * W + ax.hi) * row_bytes);
    const float w1 = ay.wl * ax.wl, w2 = ay.wl * ax.wh, w3 = ay.wh * ax.wl, w4 = ay.wh * ax.wh;
    float v1[CV], v2[CV], v3[CV], v4[CV], res[CV];
    dcn_unpack<T>(r1, ay.lo_ok && ax.lo_ok, v1);
    dcn_unpack<T>(r2, ay.lo_ok && ax.hi_ok, v2);
    dcn_unpack<T>(r3, ay.hi_ok && ax.lo_ok, v3);
    dcn_unpack<T>(r4, ay.hi_ok && ax.hi_ok, v4);
#pragma unroll
    for (int e = 0; e < CV; ++e) {
      float val = w1 * v1[e] + w2 * v2[e] + w3 * v3[e] + w4 * v4[e];
      if constexpr (MOD) val = val * mask;
      res[e] = inside ? val : 0.f;
    }
    dcn_store<T>(col + (long)m * KK * row_bytes + dcn_col_bytes<T>((long)k * Cin + c0), res);
  }
}

template <typename T>
static hipError_t launch_deform_im2col(const void* x, const float* om, void* col, long total, int M, int H, int W, int Cin, int OH, int OW,
                                       int KH, int KW, int stride, int pad, int dil, int dg, long ldo, int modulated, hipStream_t s) {
  const long blocks = (total + 255) / 256;
  const int grid = (int)(blocks > 256 * 16 ? 256 * 16 : blocks);
  if (modulated)
    hipLaunchKernelGGL((deform_im2col_kernel<T, true>), dim3(grid), dim3(256), 0, s, (const char*)x, om, (char*)col, (unsigned)total, M, H, W,
                       Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo);
  else
    hipLaunchKernelGGL((deform_im2col_kernel<T, false>), dim3(grid), dim3(256), 0, s, (const char*)x, om, (char*)col, (unsigned)total, M, H, W,
                       Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo);
  return hipGetLastError();
}

// shapes are validated by the C ABI (capi.hip: hvr_deform_im2col); `total` = M * KH * KW * (Cin / channels per lane) < 2^31 - 2^20
hipError_t run_deform_im2col(const void* x, const float* om, void* col, int B, int H, int W, int Cin, int OH, int OW, int KH, int KW, int stride,
                             int pad, int dil, int dg, long ldo, int modulated, int dtype, hipStream_t s) {
  const int M = B * OH * OW;
  const int cv = dtype == DT_F32 ? 4 : 8;
  const long total = (long)M * KH * KW * (Cin / cv);
  if (total <= 0 || total >= (1L << 31) - (1L << 20)) return hipErrorInvalidValue;   // (the grid-stride index is 32-bit)
  if (dtype == DT_BF16) return launch_deform_im2col<bf16_t>(x, om, col, total, M, H, W, Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo, modulated, s);
  if (dtype == DT_F16) return launch_deform_im2col<f16_t>(x, om, col, total, M, H, W, Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo, modulated, s);
  if (dtype == DT_F16S) return launch_deform_im2col<f16s_t>(x, om, col, total, M, H, W, Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo, modulated, s);
  return launch_deform_im2col<float>(x, om, col, total, M, H, W, Cin, OH, OW, KH, KW, stride, pad, dil, dg, ldo, modulated, s);
}

}  // namespace hvr
