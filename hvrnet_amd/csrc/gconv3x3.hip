// Grouped 3x3 convolution (ResNeXt's conv2), forward only: hvr_conv3x3_grouped (include/hvr_hip.h states the rule).
// Replaces nn.Conv2d(width, width, 3, groups=G) + BatchNorm2d(eval) + ReLU of mmdet/models/backbones/resnext.py:47-56.
//
// The work is 9 Cg MACs per output element against one read of the map and one write: it streams.  So there is no LDS and no
// barrier: a wave owns 32 output channels, keeps their weights in registers for its whole life and walks over tiles of 16 output
// pixels, loading every operand straight from the NHWC map.
//   * One 16x16x32 MFMA = [16 output channels] x [16 pixels] over K = 32.  The weights are the A operand and the pixels the B operand, so
//     a lane ends up with FOUR CONSECUTIVE CHANNELS of one pixel (D: column = lane & 15 = pixel, row = 4 (lane >> 4) + i = channel).
//   * Cg <= 16: an N tile of 16 output channels reads its own 16 input channels, K-step s holds taps 2 s and 2 s + 1 (K = 2 x 16;
//     the tenth tap is zero), five steps.  The weights are block diagonal inside the tile: a weight whose input channel lies in
//     another group of the tile is an exact zero, so every product the rule does not contain is 0 * x and the sum is the per-group
//     sum.  (The flops are 16 / Cg of the useful ones; the kernel waits for memory, not for the MFMA.)
//   * Cg == 32: K-step t is tap t over the 32 input channels of the group, nine steps; the wave's two N tiles are the two halves
//     of one group and share the pixel fragment.
//   * Loads: tap t of a tile is ONE 16-byte load per lane -- lane (r, q) takes channel chunk q of the wave's 32 channels at pixel r,
//     64 contiguous bytes per pixel.  That IS the B fragment for Cg == 32; for Cg <= 16 one v_permlane32_swap per register turns the
//     loads of taps 2 s and 2 s + 1 into the two N tiles' fragments of K-step s.  A tap outside the map and a pixel row past M load
//     the map's first bytes instead (always in bounds) and are zeroed after the load -- a zero VALUE, so that no product is 0 * inf.
//     The next tile's nine loads are issued before the current tile's MFMAs and store (two register sets).
//   * Store: acc + bias, ReLU, ONE rounding; v_permlane16_swap pairs the two N tiles' packed words so that a lane writes 16 bytes
//     (eight consecutive channels) and a pixel 64 contiguous bytes.
//   * The four waves of a workgroup take neighbouring 32-channel blocks of the same pixel tiles (C % 128 == 0: 256 contiguous bytes
//     of every pixel; else two blocks and two pixel tiles), so the halves of a 128-byte line are asked for by one workgroup.
// f32 accumulation in the MFMA, then acc + bias, ReLU and ONE rounding to the stored format.
#include "common.h"

namespace hvr {

struct GConvParams {
  const void* x; const void* w; void* y; const float* bias;
  int H, W, C, OH, OW, stride, dil, relu, cbw;   // cbw: 32-channel blocks per workgroup (4 or 2)
  long M, ntiles;
};

__device__ __forceinline__ uint4 gconv_sel(bool ok, const uint4& v) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

template <typename T, int CG>
__global__ __launch_bounds__(256) void gconv3x3_kernel(const GConvParams p) {
  constexpr bool WIDE = CG == 32;
  constexpr int STEPS = WIDE ? 9 : 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = ((int)blockIdx.y * p.cbw + wave % p.cbw) * 32;   // the wave's 32 output channels (Cg == 32: one group)
  const int ps = wave / p.cbw, PS = 4 / p.cbw;
  const T* x = reinterpret_cast<const T*>(p.x);
  const T* w = reinterpret_cast<const T*>(p.w);
  T* y = reinterpret_cast<T*>(p.y);
  const int C = p.C, H = p.H, W = p.W, OH = p.OH, OW = p.OW;

  // ---- the weights of the wave's two N tiles as A fragments: row = output channel n0 + 16 nt + r, k = 8 q + j
  uint4 wf[2][STEPS];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n0 + nt * 16 + r;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if constexpr (WIDE) {
        wf[nt][s] = *reinterpret_cast<const uint4*>(w + ((long)n * 9 + s) * 32 + 8 * q);
      } else {
        const int t = 2 * s + (q >> 1);
        uint2 h[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int c = n0 + nt * 16 + 8 * (q & 1) + 4 * e;   // input channel of this half's first element
          const bool own = t < 9 && c / CG == n / CG;
          const uint2 v = *reinterpret_cast<const uint2*>(w + ((long)n * 9 + (t < 9 ? t : 8)) * CG + (own ? c % CG : 0));
          h[e] = make_uint2(own ? v.x : 0u, own ? v.y : 0u);
        }
        wf[nt][s] = make_uint4(h[0].x, h[0].y, h[1].x, h[1].y);
      }
    }
  }
  float bias[2][4];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n0 + nt * 16 + 4 * q);
    bias[nt][0] = b4.x; bias[nt][1] = b4.y; bias[nt][2] = b4.z; bias[nt][3] = b4.w;
  }

  // ---- the pixel tiles.  Tap t of a tile is ONE load per lane: lane (r, q) takes the 16 bytes of channel chunk q of the wave's 32
  // channels at pixel r, i.e. 64 contiguous bytes per pixel and instruction.  The loads of the next tile are issued before the MFMAs
  // and stores of the current one (two register sets), so a wave always has nine loads in flight.
  const long step = (long)gridDim.x * PS;
  auto load_tile = [&](long pt, uint4 (&L)[9], unsigned& okm) {
    const long m = pt * 16 + r;
    const bool mok = m < p.M;
    const unsigned mm = mok ? (unsigned)m : 0u;          // (M < 2^31, capi.hip: two 32-bit divisions per tile, not four 64-bit ones)
    const unsigned tq = mm / (unsigned)OW, b = tq / (unsigned)OH;
    const int ox = (int)(mm - tq * (unsigned)OW), oy = (int)(tq - b * (unsigned)OH);
    const long xo = (((long)b * H + oy * p.stride) * W + ox * p.stride) * C + n0 + 8 * q;   // element offset of the centre tap
    okm = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = (t / 3 - 1) * p.dil, dx = (t % 3 - 1) * p.dil;   // (pad == dil; wave-uniform)
      const int iy = oy * p.stride + dy, ix = ox * p.stride + dx;
      const bool ok = mok && iy >= 0 && iy < H && ix >= 0 && ix < W;
      okm |= ok ? 1u << t : 0u;
      L[t] = *reinterpret_cast<const uint4*>(x + (ok ? xo + ((long)dy * W + dx) * C : 0L));
    }
  };
  uint4 cur[9], nxt[9];
  unsigned okc = 0, okn = 0;
  long pt = (long)blockIdx.x * PS + ps;
  if (pt < p.ntiles) load_tile(pt, cur, okc);
  for (; pt < p.ntiles; pt += step) {
    const bool more = pt + step < p.ntiles;   // (wave-uniform)
    if (more) load_tile(pt + step, nxt, okn);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if constexpr (WIDE) {   // chunk q of the group's 32 channels is k = 8 q .. 8 q + 7 of tap t's K-step, for both N tiles
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const uint4 v = gconv_sel((okc >> t) & 1u, cur[t]);
        acc[0] = mfma_half<T>(wf[0][t], v, acc[0]);
        acc[1] = mfma_half<T>(wf[1][t], v, acc[1]);
      }
    } else {
      // K-step s of N tile nt wants lane (r, q) to hold tap 2 s + (q >> 1), chunk q & 1 of that tile.  The loads hold tap t, tile q >> 1,
      // chunk q & 1: v_permlane32_swap of taps 2 s and 2 s + 1 (the upper half-wave of the first with the lower of the second) gives
      // {tap 2 s lower, tap 2 s + 1 lower} = tile 0's step and {tap 2 s upper, tap 2 s + 1 upper} = tile 1's, pixel r staying on its lanes.
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const uint4 a = gconv_sel((okc >> (2 * s)) & 1u, cur[2 * s]);
        const uint4 b = s < 4 ? gconv_sel((okc >> (2 * s + 1)) & 1u, cur[s < 4 ? 2 * s + 1 : 0]) : make_uint4(0u, 0u, 0u, 0u);
        const auto sx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
        const auto sz = __builtin_amdgcn_permlane32_swap(a.z, b.z, false, false);
        const auto sw = __builtin_amdgcn_permlane32_swap(a.w, b.w, false, false);
        acc[0] = mfma_half<T>(wf[0][s], make_uint4(sx[0], sy[0], sz[0], sw[0]), acc[0]);
        acc[1] = mfma_half<T>(wf[1][s], make_uint4(sx[1], sy[1], sz[1], sw[1]), acc[1]);
      }
    }
    // epilogue: lane (r, q) holds channels 4 q .. 4 q + 3 of both N tiles, 8 bytes each once rounded.  v_permlane16_swap of the two
    // (the odd 16-lane rows of tile 0's words with the even rows of tile 1's) leaves every lane with EIGHT consecutive channels of its
    // pixel -- rows 0 .. 3 hold channels 0, 16, 8, 24 onwards -- so a store is 16 bytes per lane and 64 contiguous bytes per pixel.
    uint2 pk[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[nt][i] + bias[nt][i];
        if (p.relu) v[i] = fmaxf(v[i], 0.f);
      }
      pk[nt] = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
    }
    const auto ex = __builtin_amdgcn_permlane16_swap(pk[0].x, pk[1].x, false, false);
    const auto ey = __builtin_amdgcn_permlane16_swap(pk[0].y, pk[1].y, false, false);
    const long m = pt * 16 + r;
    if (m < p.M) *reinterpret_cast<uint4*>(y + m * C + n0 + 16 * (q & 1) + 8 * (q >> 1)) = make_uint4(ex[0], ey[0], ex[1], ey[1]);
    if (more) {
#pragma unroll
      for (int t = 0; t < 9; ++t) cur[t] = nxt[t];
      okc = okn;
    }
  }
}

template <typename T, int CG> static hipError_t launch_gconv(const GConvParams& p, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((gconv3x3_kernel<T, CG>), grid, dim3(256), 0, s, p);
  return hipGetLastError();
}
template <typename T> static hipError_t launch_gconv_cg(const GConvParams& p, int Cg, dim3 grid, hipStream_t s) {
  if (Cg == 4) return launch_gconv<T, 4>(p, grid, s);
  if (Cg == 8) return launch_gconv<T, 8>(p, grid, s);
  if (Cg == 16) return launch_gconv<T, 16>(p, grid, s);
  if (Cg == 32) return launch_gconv<T, 32>(p, grid, s);
  return hipErrorInvalidValue;
}

// shapes are validated by the C ABI (capi.hip: gconv_check); dtype is DT_BF16 or DT_F16
hipError_t run_gconv3x3(const void* x, const void* w, void* y, const float* bias, int B, int H, int W, int C, int Cg, int stride, int dil, int relu,
                        int dtype, hipStream_t s) {
  GConvParams p;
  p.x = x; p.w = w; p.y = y; p.bias = bias;
  p.H = H; p.W = W; p.C = C; p.stride = stride; p.dil = dil; p.relu = relu;
  p.OH = (H - 1) / stride + 1;   // (pad == dil: the 3x3 window keeps the map's size at stride 1)
  p.OW = (W - 1) / stride + 1;
  p.M = (long)B * p.OH * p.OW;
  p.ntiles = (p.M + 15) / 16;
  p.cbw = C % 128 == 0 ? 4 : 2;
  const int gy = C / (32 * p.cbw);
  const long groups_x = (p.ntiles * p.cbw + 3) / 4;   // workgroups that give every pixel tile one wave per channel block
  const long cap = 2048 / gy > 0 ? 2048 / gy : 1;     // about eight workgroups per CU: a wave keeps its weights for several tiles
  const dim3 grid((unsigned)(groups_x < cap ? groups_x : cap), (unsigned)gy);
  if (dtype == DT_BF16) return launch_gconv_cg<bf16_t>(p, Cg, grid, s);
  if (dtype == DT_F16) return launch_gconv_cg<f16_t>(p, Cg, grid, s);
  return hipErrorInvalidValue;
}

}  // namespace hvr
