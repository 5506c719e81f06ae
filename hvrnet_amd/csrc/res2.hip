// Res2Net kernels, forward only (include/hvr_hip.h states the rules): the 3x3 conv over a channel slice of a wider NHWC map with an
// optional pre-add (hvr_res2_conv3x3: convs[i] + bns[i] + ReLU of mmdet/models/backbones/res2net_v1b.py:75-81 with `sp + spx[i]`
// folded into the operand path), the pitched average pool (hvr_avgpool_nhwc: the 'stage' pool, the shortcut pool and the carried
// slice) and the first conv of the deep stem read from the f32 NCHW image (hvr_stem3x3s2_first).
//
// The slice conv is an implicit GEMM, M = output pixels, N = Wp, K = 9 Wp, on 16x16x32 MFMAs with the weights as the A operand and
// the pixels as the B operand, so that a lane ends up with four consecutive channels of one pixel (D: column = lane & 15 = pixel,
// row = 4 (lane >> 4) + i = channel).
//   * A workgroup of eight waves owns NW output channels (32 or 64) and keeps their whole [NW][9 Wp] weight in the LDS (18 / 72 /
//     144 / 126 KB at Wp = 32 / 64 / 128 / 224): blockIdx.y picks the channel block, Wp / NW of them.  The LDS image is in fragment
//     order, [K-step][N tile][lane] 16-byte words, so staging writes and fragment reads are 1 KB contiguous per wave instruction
//     (no bank conflict); K-step s is tap s / (Wp / 32), channels 32 (s % (Wp / 32)) onwards, i.e. elements 32 s .. 32 s + 31 of a
//     weight row.
//   * The map is cut into units of 16 output pixels.  Every wave of the grid takes ONE contiguous run of `upw` units (the launch rule
//     is in run_res2_conv3x3) and walks it two units at a time: a pair shares every weight fragment read, NW / 16 LDS reads and
//     NW / 8 MFMAs per K-step and two 16-byte loads per lane.  A run of odd length ends with a single unit (its own code path: no
//     MFMA on an absent unit).  Slot = wave * gridDim.x + blockIdx.x, so that the runs that exist spread over all workgroups.
//   * Operand path: lane (r, q) loads the 16 bytes of channels 8 q .. 8 q + 7 of the K-step at pixel r straight from the pitched map
//     (64 contiguous bytes per pixel).  With `add`, the same 16 bytes of the second map are loaded, both are widened to f32, summed
//     and rounded to nearest even into the operand format: round_dtype(f32(x) + f32(add)), the operand the rule states.  A tap
//     outside the map and a pixel past M load the slice's first bytes instead (always in bounds) and are zeroed after the load
//     and the add -- a zero VALUE, so that no product is 0 * inf.
//   * Epilogue: acc + bias, ReLU, ONE rounding, 8 bytes (four channels) per lane and N tile.
#include "common.h"

namespace hvr {

struct Res2Params {
  const void* x; const void* add; void* y; const void* w; const float* bias;   // x / add / y point at channel 0 of their slices
  long ldx, lda, ldy;
  int H, W, OH, OW, stride, dil, relu;
  int M, nunits, upw;
};

constexpr int kRes2Waves = 8;

template <typename T> __device__ __forceinline__ uint4 res2_add8(const uint4& a, const uint4& b) {
  float a0, a1, b0, b1;
  uint4 o;
  unpack2<T>(a.x, a0, a1); unpack2<T>(b.x, b0, b1); o.x = pack2<T>(a0 + b0, a1 + b1);
  unpack2<T>(a.y, a0, a1); unpack2<T>(b.y, b0, b1); o.y = pack2<T>(a0 + b0, a1 + b1);
  unpack2<T>(a.z, a0, a1); unpack2<T>(b.z, b0, b1); o.z = pack2<T>(a0 + b0, a1 + b1);
  unpack2<T>(a.w, a0, a1); unpack2<T>(b.w, b0, b1); o.w = pack2<T>(a0 + b0, a1 + b1);
  return o;
}

template <typename T, int WP, int NW, bool ADD>
__global__ __launch_bounds__(kRes2Waves * 64, WP <= 64 ? 4 : 2) void res2_conv3x3_kernel(const Res2Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = NW / 16, KC = WP / 32, STEPS = 9 * KC;
  uint4* wl = reinterpret_cast<uint4*>(smem);   // [STEPS][NT][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = (int)blockIdx.y * NW;
  const T* x = reinterpret_cast<const T*>(p.x);
  const T* ad = reinterpret_cast<const T*>(p.add);
  const T* w = reinterpret_cast<const T*>(p.w);
  T* y = reinterpret_cast<T*>(p.y);

  // ---- the workgroup's weights into the LDS, as A fragments: row = output channel n0 + 16 nt + r, k = 32 s + 8 q + j
#pragma unroll 6
  for (int idx = wave; idx < STEPS * NT; idx += kRes2Waves) {
    const int s = idx / NT, nt = idx % NT;
    wl[idx * 64 + lane] = *reinterpret_cast<const uint4*>(w + (long)(n0 + nt * 16 + r) * (9 * WP) + s * 32 + 8 * q);
  }
  float bias[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n0 + nt * 16 + 4 * q);
    bias[nt][0] = b4.x; bias[nt][1] = b4.y; bias[nt][2] = b4.z; bias[nt][3] = b4.w;
  }
  __syncthreads();

  const int H = p.H, W = p.W, OH = p.OH, OW = p.OW;
  const long slot = (long)wave * gridDim.x + blockIdx.x;
  const long u0 = slot * p.upw;
  const long u1 = u0 + p.upw < p.nunits ? u0 + p.upw : p.nunits;

  auto pair = [&](long u, auto two_c) {
    constexpr int G = decltype(two_c)::value ? 2 : 1;
    bool mok[G];
    int iy0[G], ix0[G];
    long px[G], mo[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const long m = (u + g) * 16 + r;
      mok[g] = m < p.M;
      const unsigned mm = mok[g] ? (unsigned)m : 0u;     // (M < 2^31: two 32-bit divisions per unit)
      const unsigned tq = mm / (unsigned)OW, b = tq / (unsigned)OH;
      const int ox = (int)(mm - tq * (unsigned)OW), oy = (int)(tq - b * (unsigned)OH);
      iy0[g] = oy * p.stride; ix0[g] = ox * p.stride;
      px[g] = ((long)b * H + iy0[g]) * W + ix0[g];        // pixel index of the centre tap
      mo[g] = m;
    }
    f32x4 acc[G][NT];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[g][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = (t / 3 - 1) * p.dil, dx = (t % 3 - 1) * p.dil;   // (pad == dil; wave-uniform)
      bool ok[G];
      long xo[G], ao[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int iy = iy0[g] + dy, ix = ix0[g] + dx;
        ok[g] = mok[g] && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const long pp = ok[g] ? px[g] + (long)dy * W + dx : 0L;
        xo[g] = pp * p.ldx + 8 * q;
        ao[g] = pp * p.lda + 8 * q;
      }
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        uint4 bf[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          uint4 v = *reinterpret_cast<const uint4*>(x + xo[g] + kc * 32);
          if constexpr (ADD) v = res2_add8<T>(v, *reinterpret_cast<const uint4*>(ad + ao[g] + kc * 32));
          bf[g] = make_uint4(ok[g] ? v.x : 0u, ok[g] ? v.y : 0u, ok[g] ? v.z : 0u, ok[g] ? v.w : 0u);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const uint4 a = wl[((t * KC + kc) * NT + nt) * 64 + lane];
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g][nt] = mfma_half<T>(a, bf[g], acc[g][nt]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (mok[g]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = acc[g][nt][i] + bias[nt][i];
            if (p.relu) v[i] = fmaxf(v[i], 0.f);
          }
          *reinterpret_cast<uint2*>(y + mo[g] * p.ldy + n0 + nt * 16 + 4 * q) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
        }
      }
    }
  };

  for (long u = u0; u < u1; u += 2) {   // (wave-uniform)
    if (u + 1 < u1) pair(u, std::true_type{});
    else pair(u, std::false_type{});
  }
}

template <typename T, int WP, int NW, bool ADD> static hipError_t launch_res2(const Res2Params& p, dim3 grid, hipStream_t s) {
  constexpr int lds = 9 * (WP / 32) * (NW / 16) * 1024;
  static std::atomic<unsigned> attr_set_dev{0};   // (the attribute is per device)
  per_device_once(attr_set_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(res2_conv3x3_kernel<T, WP, NW, ADD>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  hipLaunchKernelGGL((res2_conv3x3_kernel<T, WP, NW, ADD>), grid, dim3(kRes2Waves * 64), lds, s, p);
  return hipGetLastError();
}

// output channels per workgroup: the widest block whose weights fit the 160 KB of LDS
static int res2_nw(int Wp) { return Wp == 32 ? 32 : Wp == 64 ? 64 : Wp == 128 ? 64 : 32; }

template <typename T, bool ADD> static hipError_t launch_res2_wp(const Res2Params& p, int Wp, dim3 grid, hipStream_t s) {
  if (Wp == 32) return launch_res2<T, 32, 32, ADD>(p, grid, s);
  if (Wp == 64) return launch_res2<T, 64, 64, ADD>(p, grid, s);
  if (Wp == 128) return launch_res2<T, 128, 64, ADD>(p, grid, s);
  if (Wp == 224) return launch_res2<T, 224, 32, ADD>(p, grid, s);
  return hipErrorInvalidValue;
}

// The launch rule.  Units of 16 output pixels: nunits = ceil(M / 16).  grid = (gx, Wp / NW) with gx = min(ceil(nunits / 16), cap),
// cap = max(1, 256 wpc / (Wp / NW)) and wpc = 2 workgroups per CU at Wp <= 64 (72 KB of LDS or less), else 1; a wave takes
// upw = ceil(nunits / (8 gx)) consecutive units from unit (wave * gx + blockIdx.x) * upw on, two at a time.
// Shapes are validated by the C ABI (capi.hip: res2_check); dtype is DT_BF16 or DT_F16; x / add / y point at their slices.
hipError_t run_res2_conv3x3(const void* x, long ldx, const void* add, long lda, void* y, long ldy, const void* w, const float* bias, int B, int H,
                            int W, int Wp, int stride, int dil, int relu, int dtype, hipStream_t s) {
  Res2Params p;
  p.x = x; p.add = add; p.y = y; p.w = w; p.bias = bias;
  p.ldx = ldx; p.lda = lda; p.ldy = ldy;
  p.H = H; p.W = W; p.stride = stride; p.dil = dil; p.relu = relu;
  p.OH = (H - 1) / stride + 1;   // (pad == dil: the 3x3 window keeps the map's size at stride 1)
  p.OW = (W - 1) / stride + 1;
  p.M = (int)((long)B * p.OH * p.OW);
  p.nunits = (p.M + 15) / 16;
  const int gy = Wp / res2_nw(Wp);
  const int wpc = Wp <= 64 ? 2 : 1;
  const int cap = 256 * wpc / gy > 0 ? 256 * wpc / gy : 1;
  const int want = (p.nunits + 15) / 16;
  const int gx = want < cap ? want : cap;
  p.upw = (p.nunits + kRes2Waves * gx - 1) / (kRes2Waves * gx);
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (dtype == DT_BF16) return add ? launch_res2_wp<bf16_t, true>(p, Wp, grid, s) : launch_res2_wp<bf16_t, false>(p, Wp, grid, s);
  if (dtype == DT_F16) return add ? launch_res2_wp<f16_t, true>(p, Wp, grid, s) : launch_res2_wp<f16_t, false>(p, Wp, grid, s);
  return hipErrorInvalidValue;
}

// ---- average pool over a channel slice: f32 sum in raster tap order, times the reciprocal of the divisor, one rounding
struct PoolParams {
  const void* x; void* y;
  long ldx, ldy, total;
  int H, W, OH, OW, C4, k, stride, pad, include_pad;
};

template <typename T> __global__ __launch_bounds__(256) void avgpool_kernel(const PoolParams p) {
  const T* x = reinterpret_cast<const T*>(p.x);
  T* y = reinterpret_cast<T*>(p.y);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % p.C4);
    const long m = i / p.C4;
    const int ox = (int)(m % p.OW);
    const long tq = m / p.OW;
    const int oy = (int)(tq % p.OH);
    const long b = tq / p.OH;
    int h0 = oy * p.stride - p.pad, w0 = ox * p.stride - p.pad;
    int h1 = min(h0 + p.k, p.H + p.pad), w1 = min(w0 + p.k, p.W + p.pad);
    const int full = (h1 - h0) * (w1 - w0);   // the window clipped to the padded map: the divisor with count_include_pad
    h0 = max(h0, 0); w0 = max(w0, 0); h1 = min(h1, p.H); w1 = min(w1, p.W);
    const int div = p.include_pad ? full : (h1 - h0) * (w1 - w0);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    bool first = true;
    for (int iy = h0; iy < h1; ++iy)
      for (int ix = w0; ix < w1; ++ix) {
        float v[4];
        load4(x + ((b * p.H + iy) * p.W + ix) * p.ldx + 4 * c4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = first ? v[j] : s[j] + v[j];   // (the first tap as it is: a 1x1 window copies -0.0 too)
        first = false;
      }
    const float rinv = 1.f / (float)(div > 0 ? div : 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] *= rinv;
    store4(y + m * p.ldy + 4 * c4, s);
  }
}

// shapes are validated by the C ABI (capi.hip: hvr_avgpool_nhwc); dtype is DT_F32, DT_BF16 or DT_F16; x / y point at their slices
hipError_t run_avgpool(const void* x, long ldx, void* y, long ldy, int B, int H, int W, int OH, int OW, int C, int k, int stride, int pad,
                       int include_pad, int dtype, hipStream_t s) {
  PoolParams p;
  p.x = x; p.y = y; p.ldx = ldx; p.ldy = ldy;
  p.H = H; p.W = W; p.OH = OH; p.OW = OW; p.C4 = C / 4; p.k = k; p.stride = stride; p.pad = pad; p.include_pad = include_pad;
  p.total = (long)B * OH * OW * p.C4;
  const long blocks = (p.total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
  if (dtype == DT_BF16) hipLaunchKernelGGL(avgpool_kernel<bf16_t>, grid, dim3(256), 0, s, p);
  else if (dtype == DT_F16) hipLaunchKernelGGL(avgpool_kernel<f16_t>, grid, dim3(256), 0, s, p);
  else if (dtype == DT_F32) hipLaunchKernelGGL(avgpool_kernel<float>, grid, dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- the first conv of the deep stem (res2net_v1b.py:174-177: Conv 3 -> 32, 3x3 / 2, pad 1 + BN + ReLU) from the f32 NCHW image.
// K = 27: a lane computes one output pixel's 32 channels with f32 FMAs (bias first, then taps in (ky, kx, c) order), the weights
// are wave-uniform.  It writes ldy channels per pixel: the 32 results and exact zeros behind them (the K padding of the next conv).
template <typename T> __global__ __launch_bounds__(256) void stem3x3s2_first_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                                                   const float* __restrict__ bias, T* __restrict__ y, int H, int W,
                                                                                   int OH, int OW, int ldy, long M) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int ox = (int)(m % OW);
  const long tq = m / OW;
  const int oy = (int)(tq % OH);
  const long b = tq / OH;
  float in[27];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
      for (int c = 0; c < 3; ++c) in[(ky * 3 + kx) * 3 + c] = ok ? img[((b * 3 + c) * H + iy) * W + ix] : 0.f;
    }
  T* yo = y + m * ldy;
#pragma unroll
  for (int n4 = 0; n4 < 8; ++n4) {
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bias[n4 * 4 + j];
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(in[k], w[(n4 * 4 + j) * 27 + k], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaxf(acc[j], 0.f);
    store4(yo + n4 * 4, acc);
  }
  const float z[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 32; c < ldy; c += 4) store4(yo + c, z);
}

// dtype of y: DT_F32, DT_BF16 or DT_F16 (validated by the C ABI)
hipError_t run_stem3x3s2_first(const float* img, const float* w, const float* bias, void* y, int B, int H, int W, int ldy, int dtype, hipStream_t s) {
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;   // (H + 2 - 3) / 2 + 1
  const long M = (long)B * OH * OW;
  const dim3 grid((unsigned)((M + 255) / 256));
  if (dtype == DT_BF16) hipLaunchKernelGGL(stem3x3s2_first_kernel<bf16_t>, grid, dim3(256), 0, s, img, w, bias, (bf16_t*)y, H, W, OH, OW, ldy, M);
  else if (dtype == DT_F16) hipLaunchKernelGGL(stem3x3s2_first_kernel<f16_t>, grid, dim3(256), 0, s, img, w, bias, (f16_t*)y, H, W, OH, OW, ldy, M);
  else if (dtype == DT_F32) hipLaunchKernelGGL(stem3x3s2_first_kernel<float>, grid, dim3(256), 0, s, img, w, bias, (float*)y, H, W, OH, OW, ldy, M);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hvr
