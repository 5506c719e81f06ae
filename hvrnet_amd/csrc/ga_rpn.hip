// Guided Anchoring RPN (GA-RPN), inference: location mask + offset conv, masked conv, guided proposal selection.
// Replaces mmdet/models/anchor_heads/guided_anchor_head.py:197-208 (mask, feature_adaption.conv_offset), :271-362 (get_anchors,
// get_guided_anchors_single, use_loc_filter=True), mmdet/ops/masked_conv/masked_conv.py:15-53 (MaskedConv2dFunction.forward)
// and mmdet/models/anchor_heads/ga_rpn_head.py:60-127 (get_bboxes_single) for one level.  The rules are stated step by step in
// include/hvr_hip.h; the f64 statements the tests compare with are tests/ga_rpn_refs.py.
//   * ga_mask_offsets_kernel   one thread per (pixel, offset channel): the K = 2 product is two multiplies and one add in f32
//                              (no MFMA shape); the thread of channel 0 also writes the pixel's keep byte.
//   * masked_conv_kernel       one wave per output pixel.  An unkept pixel costs one byte read and Cout zero stores: its rows
//                              of x are never fetched.  A kept pixel: every lane walks the taps inside the map and its own
//                              16-byte channel chunks (lane, lane + 64, ...), Cout f32 accumulators per lane, then a fixed butterfly
//                              over the wave (xor 32, 16, 8, 4, 2, 1): the same sum order for every pixel, no atomics, one store.
//                              The weights (Cout * K elements, 10 KB for the 1 + 4 heads at K = 1024 bf16) are re-read through
//                              the vector cache; x is the only operand that comes from memory.
//   * ga_select_kernel         one workgroup per frame: keys of the kept pixels (sigmoid of cls, index ascending on ties) sorted
//                              in LDS, the first min(kept, nms_pre) decoded twice (square -> guided anchor -> proposal) into a
//                              score-sorted list, rows behind them zero.  The NMS is run_nms_batched of nms.hip on that list.
//   * ga_gather_kernel         the survivors that are real candidates (zero rows sort last and never suppress a real box),
//                              the first nms_post of them in the reference's list order (score order behind a top-k, else
//                              row-major), then the top max_num of those by score.
// Built with -ffp-contract=off (build.sh): every product and sum of the box arithmetic is rounded on its own; the masked conv
// names its fused multiply-adds explicitly.
#include "nms_dev.h"
#include "ga_rpn.h"

namespace hvr {

// ---------------------------------------------------------------------------------
// location mask + offset conv
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ga_mask_offsets_kernel(const float* __restrict__ loc, long loc_pitch, float thr,
                                                              unsigned char* __restrict__ keep, const float* __restrict__ shape,
                                                              long shape_pitch, const float* __restrict__ w, float* __restrict__ om,
                                                              long ldo, int nch, long P) {
  const long total = P * (long)nch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long p = idx / nch;
    const int c = (int)(idx - p * nch);
    if (keep && c == 0) {
      const float s = 1.f / (1.f + expf(-loc[p * loc_pitch]));   // torch.sigmoid: precise expf, rounded add and divide
      keep[p] = s >= thr ? 1 : 0;
    }
    if (om) {
      const float s0 = shape[p * shape_pitch], s1 = shape[p * shape_pitch + 1];
      om[p * ldo + c] = w[2 * c] * s0 + w[2 * c + 1] * s1;
    }
  }
}

hipError_t run_ga_mask_offsets(const float* loc, long loc_pitch, float thr, unsigned char* keep, const float* shape, long shape_pitch,
                               const float* w, float* om, long ldo, int nch, long P, hipStream_t s) {
  const long total = P * (long)nch;
  const long blocks = (total + 255) / 256;
  const int grid = (int)(blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(ga_mask_offsets_kernel, dim3(grid), dim3(256), 0, s, loc, loc_pitch, thr, keep, shape, shape_pitch, w, om, ldo, nch, P);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// masked conv
// ---------------------------------------------------------------------------------
template <typename T> struct McVec;   // elements of one 16-byte chunk
template <> struct McVec<float> { static constexpr int kCV = 4; };
template <> struct McVec<bf16_t> { static constexpr int kCV = 8; };
template <> struct McVec<f16_t> { static constexpr int kCV = 8; };

template <typename T> __device__ __forceinline__ void mc_load(const T* p, float* f) {
  const uint4 a = *reinterpret_cast<const uint4*>(p);
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
  } else {
    unpack2<T>(a.x, f[0], f[1]); unpack2<T>(a.y, f[2], f[3]); unpack2<T>(a.z, f[4], f[5]); unpack2<T>(a.w, f[6], f[7]);
  }
}

constexpr int MC_MAX_COUT = 8;
constexpr int MC_WAVES = 4;

template <typename T, int NO>
__global__ __launch_bounds__(64 * MC_WAVES) void masked_conv_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                                   const float* __restrict__ bias, const unsigned char* __restrict__ keep,
                                                                   float* __restrict__ out, long P, int H, int W, int Cin, int KS, int pad,
                                                                   long ldo) {
  constexpr int CV = McVec<T>::kCV;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * MC_WAVES + (threadIdx.x >> 6), nwave = (long)gridDim.x * MC_WAVES;
  const long K = (long)KS * KS * Cin;
  for (long p = wave; p < P; p += nwave) {
    float* o = out + p * ldo;
    if (!keep[p]) {            // wave-uniform: new_zeros of the reference, and no read of x
      if (lane < NO) o[lane] = 0.f;
      continue;
    }
    const int px = (int)(p % W);
    const long t = p / W;
    const int py = (int)(t % H);
    const long b = t / H;
    float acc[NO];
#pragma unroll
    for (int n = 0; n < NO; ++n) acc[n] = 0.f;
    for (int kh = 0; kh < KS; ++kh) {
      const int iy = py - pad + kh;
      if (iy < 0 || iy >= H) continue;
      for (int kw = 0; kw < KS; ++kw) {
        const int ix = px - pad + kw;
        if (ix < 0 || ix >= W) continue;
        const T* xr = x + ((b * H + iy) * W + ix) * (long)Cin;
        const T* wr = w + (long)(kh * KS + kw) * Cin;
        for (int c0 = lane * CV; c0 < Cin; c0 += 64 * CV) {
          float xv[CV];
          mc_load<T>(xr + c0, xv);
#pragma unroll
          for (int n = 0; n < NO; ++n) {
            float wv[CV];
            mc_load<T>(wr + n * K + c0, wv);
#pragma unroll
            for (int e = 0; e < CV; ++e) acc[n] = __builtin_fmaf(xv[e], wv[e], acc[n]);
          }
        }
      }
    }
#pragma unroll
    for (int n = 0; n < NO; ++n) {
      float v = acc[n];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
      acc[n] = v;
    }
    float mine = 0.f;
#pragma unroll
    for (int n = 0; n < NO; ++n) mine = lane == n ? acc[n] : mine;
    if (lane < NO) o[lane] = mine + (bias ? bias[lane] : 0.f);
  }
}

template <typename T, int NO>
static hipError_t launch_masked_conv(const void* x, const void* w, const float* bias, const unsigned char* keep, float* out, long P, int H,
                                     int W, int Cin, int KS, int pad, long ldo, hipStream_t s) {
  const long blocks = (P + MC_WAVES - 1) / MC_WAVES;
  const int grid = (int)(blocks > 256 * 16 ? 256 * 16 : blocks);
  hipLaunchKernelGGL((masked_conv_kernel<T, NO>), dim3(grid), dim3(64 * MC_WAVES), 0, s, (const T*)x, (const T*)w, bias, keep, out, P, H, W,
                     Cin, KS, pad, ldo);
  return hipGetLastError();
}

template <typename T>
static hipError_t masked_conv_by_cout(const void* x, const void* w, const float* bias, const unsigned char* keep, float* out, long P, int H,
                                      int W, int Cin, int Cout, int KS, int pad, long ldo, hipStream_t s) {
  switch (Cout) {
    case 1: return launch_masked_conv<T, 1>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 2: return launch_masked_conv<T, 2>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 3: return launch_masked_conv<T, 3>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 4: return launch_masked_conv<T, 4>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 5: return launch_masked_conv<T, 5>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 6: return launch_masked_conv<T, 6>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 7: return launch_masked_conv<T, 7>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
    case 8: return launch_masked_conv<T, 8>(x, w, bias, keep, out, P, H, W, Cin, KS, pad, ldo, s);
  }
  return hipErrorInvalidValue;
}

int masked_conv_max_cout() { return MC_MAX_COUT; }

// shapes are validated by the C ABI (capi.hip: hvr_masked_conv_fwd)
hipError_t run_masked_conv(const void* x, const void* w, const float* bias, const unsigned char* keep, float* out, int B, int H, int W,
                           int Cin, int Cout, int KS, int pad, long ldo, int dtype, hipStream_t s) {
  const long P = (long)B * H * W;
  if (dtype == DT_BF16) return masked_conv_by_cout<bf16_t>(x, w, bias, keep, out, P, H, W, Cin, Cout, KS, pad, ldo, s);
  if (dtype == DT_F16) return masked_conv_by_cout<f16_t>(x, w, bias, keep, out, P, H, W, Cin, Cout, KS, pad, ldo, s);
  if (dtype == DT_F32) return masked_conv_by_cout<float>(x, w, bias, keep, out, P, H, W, Cin, Cout, KS, pad, ldo, s);
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------
// guided proposals: select + decode, one workgroup per frame
// ---------------------------------------------------------------------------------
// delta2bbox (mmdet/core/bbox/transforms.py:78-110) without the clip to the image: box a, deltas d already denormalised
__device__ __forceinline__ void ga_delta2bbox(const float a[4], float dx, float dy, float dw, float dh, float max_ratio, float o[4]) {
  dw = fminf(fmaxf(dw, -max_ratio), max_ratio);
  dh = fminf(fmaxf(dh, -max_ratio), max_ratio);
  const float px = (a[0] + a[2]) * 0.5f, py = (a[1] + a[3]) * 0.5f, pw = a[2] - a[0] + 1.0f, ph = a[3] - a[1] + 1.0f;
  const float gw = pw * expf(dw), gh = ph * expf(dh), gx = px + pw * dx, gy = py + ph * dy;
  o[0] = gx - gw * 0.5f + 0.5f;
  o[1] = gy - gh * 0.5f + 0.5f;
  o[2] = gx + gw * 0.5f - 0.5f;
  o[3] = gy + gh * 0.5f - 0.5f;
}

// cls [T][HW] (pitch cls_pitch), reg [T][HW][4] (pitch reg_pitch), shape [T][HW][2] (pitch shape_pitch), keep [T][HW]
// props [T][npre][5]: the candidates in (score desc, pixel asc) order, rows from ncand[f] on zero
__global__ __launch_bounds__(1024) void ga_select_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
                                                         const float* __restrict__ shape, const unsigned char* __restrict__ keep,
                                                         float* __restrict__ props, int* __restrict__ pix, int* __restrict__ ncand,
                                                         int* __restrict__ topk, const GaParams gp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* comp = reinterpret_cast<unsigned long long*>(smem);   // [np2] key << 32 | ~pixel, 0 for unkept / pad
  __shared__ int sh_kept;
  const int f = blockIdx.x, n = gp.H * gp.W, np2 = next_pow2(n);
  const float* c = cls + (long)f * n * gp.cls_pitch;
  const float* r = reg + (long)f * n * gp.reg_pitch;
  const float* sp = shape + (long)f * n * gp.shape_pitch;
  const unsigned char* kp = keep + (long)f * n;
  if (threadIdx.x == 0) sh_kept = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < np2; i += blockDim.x) {
    unsigned long long v = 0ull;
    if (i < n && kp[i]) {
      const float s = 1.f / (1.f + expf(-c[(long)i * gp.cls_pitch]));   // torch.sigmoid
      v = ((unsigned long long)float_key(s) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
      ++mine;
    }
    comp[i] = v;
  }
  if (mine) atomicAdd(&sh_kept, mine);
  __syncthreads();
  const int kept = sh_kept;
  block_sort_desc_u64(comp, np2);
  __syncthreads();
  const int nc = (gp.nms_pre > 0 && kept > gp.nms_pre) ? gp.nms_pre : kept;   // <= npre
  for (int j = threadIdx.x; j < gp.npre; j += blockDim.x) {
    float* o = props + ((long)f * gp.npre + j) * 5;
    if (j >= nc) {
      o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
      pix[(long)f * gp.npre + j] = 0x7fffffff;
      continue;
    }
    const int i = (int)(0xffffffffu - (uint32_t)(comp[j] & 0xffffffffull));
    pix[(long)f * gp.npre + j] = i;
    const int x = i % gp.W, y = i / gp.W;
    const float sq[4] = {gp.square[0] + x * gp.stride, gp.square[1] + y * gp.stride, gp.square[2] + x * gp.stride,
                         gp.square[3] + y * gp.stride};
    // guided anchor: deltas (0, 0, shape0, shape1), denormalised with the anchoring means / stds (the means reach dx, dy)
    const float s0 = sp[(long)i * gp.shape_pitch], s1 = sp[(long)i * gp.shape_pitch + 1];
    float an[4], box[4];
    ga_delta2bbox(sq, 0.f * gp.as[0] + gp.am[0], 0.f * gp.as[1] + gp.am[1], s0 * gp.as[2] + gp.am[2], s1 * gp.as[3] + gp.am[3],
                  gp.a_ratio, an);
    const float* d = r + (long)i * gp.reg_pitch;
    ga_delta2bbox(an, d[0] * gp.ts[0] + gp.tm[0], d[1] * gp.ts[1] + gp.tm[1], d[2] * gp.ts[2] + gp.tm[2], d[3] * gp.ts[3] + gp.tm[3],
                  gp.t_ratio, box);
    o[0] = fminf(fmaxf(box[0], 0.f), gp.img_w - 1.f);
    o[1] = fminf(fmaxf(box[1], 0.f), gp.img_h - 1.f);
    o[2] = fminf(fmaxf(box[2], 0.f), gp.img_w - 1.f);
    o[3] = fminf(fmaxf(box[3], 0.f), gp.img_h - 1.f);
    o[4] = 1.f / (1.f + expf(-c[(long)i * gp.cls_pitch]));
  }
  if (threadIdx.x == 0) {
    ncand[f] = nc;
    topk[f] = (gp.nms_pre > 0 && kept > gp.nms_pre) ? 1 : 0;
  }
}

// keep [T][npre]: the survivors' positions in the score-sorted list, ascending; those below ncand[f] are real candidates (they come
// first).  "The first nms_post" of the reference are the first in ITS candidate list (ga_rpn_head.py:114-115 on the CPU NMS, which
// returns the survivors by ascending input index, as rpn_gather_kernel of nms.hip reads it): score order when the top nms_pre were
// taken (topk[f]), row-major pixel order when they were not.  Then the top max_num by score: positions ascending.
__global__ __launch_bounds__(256) void ga_gather_kernel(const float* __restrict__ props, const long long* __restrict__ keep,
                                                        const int* __restrict__ n_keep, const int* __restrict__ pix,
                                                        const int* __restrict__ ncand, const int* __restrict__ topk, int npre,
                                                        int nms_post, int max_num, float* __restrict__ out, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* comp = reinterpret_cast<unsigned long long*>(smem);   // [next_pow2(survivors)]
  __shared__ int sh_cnt;
  const int f = blockIdx.x;
  const float* pf = props + (long)f * npre * 5;
  const long long* kf = keep + (long)f * npre;
  const int* xf = pix + (long)f * npre;
  int nk = n_keep[f];
  nk = nk < npre ? nk : npre;
  const int nc = ncand[f];
  if (threadIdx.x == 0) sh_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < nk; i += blockDim.x) mine += kf[i] < nc ? 1 : 0;
  if (mine) atomicAdd(&sh_cnt, mine);
  __syncthreads();
  const int cnt = sh_cnt;
  const int take = cnt < nms_post ? cnt : nms_post;
  const int num = take < max_num ? take : max_num;
  const bool by_pixel = !topk[f] && cnt > take;    // (every survivor is taken: nothing to choose, the list order is the score order)
  if (by_pixel) {
    const int p2 = next_pow2(cnt);
    for (int i = threadIdx.x; i < p2; i += blockDim.x) {
      unsigned long long v = 0ull;
      if (i < cnt) {
        const uint32_t pos = (uint32_t)kf[i];
        v = ((unsigned long long)(0xffffffffu - (uint32_t)xf[pos]) << 32) | (unsigned long long)(0xffffffffu - pos);
      }
      comp[i] = v;
    }
    __syncthreads();
    block_sort_desc_u64(comp, p2);      // ascending pixel
    __syncthreads();
    const int t2 = next_pow2(take);
    for (int i = threadIdx.x; i < t2; i += blockDim.x) {
      const unsigned long long v = comp[i];
      comp[i] = i < take ? ((v & 0xffffffffull) << 32) | 1ull : 0ull;   // key = ~position: descending == ascending position
    }
    __syncthreads();
    block_sort_desc_u64(comp, t2);
    __syncthreads();
  }
  for (int j = threadIdx.x; j < num * 5; j += blockDim.x) {
    const int row = j / 5, col = j - row * 5;
    const long pos = by_pixel ? (long)(0xffffffffu - (uint32_t)(comp[row] >> 32)) : (long)kf[row];
    out[((long)f * max_num + row) * 5 + col] = pf[pos * 5 + col];
  }
  if (threadIdx.x == 0) counts[f] = num;
}

hipError_t run_ga_select(const float* cls, const float* reg, const float* shape, const unsigned char* keep, float* props, int* pix,
                         int* ncand, int* topk, const GaParams& gp, hipStream_t s) {
  int np2 = 1;
  while (np2 < gp.H * gp.W) np2 <<= 1;
  if (np2 > 8192) return hipErrorInvalidValue;
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8);
  });
  hipLaunchKernelGGL(ga_select_kernel, dim3(gp.T), dim3(1024), (size_t)np2 * 8, s, cls, reg, shape, keep, props, pix, ncand, topk, gp);
  return hipGetLastError();
}

hipError_t run_ga_gather(const float* props, const long long* keep, const int* n_keep, const int* pix, const int* ncand, const int* topk,
                         int T, int npre, int nms_post, int max_num, float* out, int* counts, hipStream_t s) {
  int np2 = 1;
  while (np2 < npre) np2 <<= 1;
  if (np2 > 8192) return hipErrorInvalidValue;
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ga_gather_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8);
  });
  hipLaunchKernelGGL(ga_gather_kernel, dim3(T), dim3(256), (size_t)np2 * 8, s, props, keep, n_keep, pix, ncand, topk, npre, nms_post, max_num,
                     out, counts);
  return hipGetLastError();
}

}  // namespace hvr
