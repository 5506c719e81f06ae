// Device helpers of the NMS kernels shared by nms.hip and tta.hip: the score sort (descending score, ascending index on ties) and the
// IoU threshold test with the CPU reference's arithmetic.  Included by value into each translation unit (no relocatable device code).
#pragma once
#include "common.h"

namespace hvr {

__device__ __forceinline__ uint32_t float_key(float f) {  // ascending uint == ascending float
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// In-LDS bitonic sort of n_pow2 (key, idx) pairs: descending key, ascending idx on ties.
// Pad entries must carry key 0 / idx 0xffffffff so they sink to the end.
__device__ __forceinline__ bool pair_before(uint32_t ka, uint32_t ia, uint32_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}
__device__ void bitonic_sort_pairs(uint32_t* key, uint32_t* idx, int n_pow2) {
  for (int k = 2; k <= n_pow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t ka = key[i], ia = idx[i], kb = key[ixj], ib = idx[ixj];
          const bool up = (i & k) == 0;  // this sub-sequence sorts "first before last"
          const bool swap = up ? pair_before(kb, ib, ka, ia) : pair_before(ka, ia, kb, ib);
          if (swap) { key[i] = kb; idx[i] = ib; key[ixj] = ka; idx[ixj] = ia; }
        }
      }
      __syncthreads();
    }
  }
}

// Descending sort of n_pow2 64-bit composites (key << 32 | 0xffffffff - index: higher key first, lower index on ties; pads
// are 0 and sink to the end) by a 1024-thread workgroup, the same bitonic network as above with most of it off the LDS:
// thread t holds elements m * 1024 + t (m < E) in registers, so partners at distance j >= 1024 are its own registers, at
// j < 64 a lane of its own wave (shuffles, no barrier), and only 64 <= j < 1024 goes through the LDS (22 of the 91 stages at
// n = 8192; the in-LDS version pays two array reads, a conditional write and a barrier in every one of the 91).
template <int E>
__device__ __forceinline__ void block_sort_desc_u64_regs(unsigned long long* buf) {
  constexpr int B = 1024;
  const int t = threadIdx.x;
  unsigned long long v[E];
#pragma unroll
  for (int m = 0; m < E; ++m) v[m] = buf[m * B + t];
  for (int k = 2; k <= E * B; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= B) {
#pragma unroll
        for (int jm = E / 2; jm > 0; jm >>= 1) {  // register indices stay compile-time constants
          if (j != jm * B) continue;
#pragma unroll
          for (int m = 0; m < E; ++m) {
            const int pm = m ^ jm;
            if (pm > m) {
              const bool up = ((m * B) & k) == 0;
              const unsigned long long a = v[m], b = v[pm];
              const unsigned long long hi = a > b ? a : b, lo = a > b ? b : a;
              v[m] = up ? hi : lo;
              v[pm] = up ? lo : hi;
            }
          }
        }
      } else if (j >= 64) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) buf[m * B + t] = v[m];
        __syncthreads();
        const bool lower = (t & j) == 0;
#pragma unroll
        for (int m = 0; m < E; ++m) {
          const unsigned long long o = buf[m * B + (t ^ j)];
          const bool up = ((m * B + t) & k) == 0;
          const bool keep_max = lower == up;
          const unsigned long long a = v[m];
          v[m] = keep_max ? (a > o ? a : o) : (a > o ? o : a);
        }
      } else {
        const bool lower = (t & j) == 0;
#pragma unroll
        for (int m = 0; m < E; ++m) {
          const unsigned long long a = v[m];
          const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)a, j), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(a >> 32), j);
          const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
          const bool up = ((m * B + t) & k) == 0;
          const bool keep_max = lower == up;
          v[m] = keep_max ? (a > o ? a : o) : (a > o ? o : a);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < E; ++m) buf[m * B + t] = v[m];
  __syncthreads();
}

// any workgroup size / length: the plain in-LDS network
__device__ void block_sort_desc_u64(unsigned long long* buf, int n_pow2) {
  if (blockDim.x == 1024 && n_pow2 >= 1024 && n_pow2 <= 8192) {
    switch (n_pow2 >> 10) {
      case 1: block_sort_desc_u64_regs<1>(buf); return;
      case 2: block_sort_desc_u64_regs<2>(buf); return;
      case 4: block_sort_desc_u64_regs<4>(buf); return;
      case 8: block_sort_desc_u64_regs<8>(buf); return;
    }
  }
  for (int k = 2; k <= n_pow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = buf[i], b = buf[ixj];
          const bool up = (i & k) == 0;
          if (up ? (b > a) : (a > b)) { buf[i] = b; buf[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int next_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

__device__ __forceinline__ float box_iou_plus1(const float4 a, const float4 b) {
  // nms_cpu.cpp:18,46-54 (same arithmetic order; "+1" pixel convention)
  const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y), xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
  const float w = fmaxf(0.f, xx2 - xx1 + 1.f), h = fmaxf(0.f, yy2 - yy1 + 1.f);
  const float inter = w * h;
  const float aa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f), ab = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
  return inter / (aa + ab - inter);
}

__device__ __forceinline__ float box_area_plus1(const float4 a) { return (a.z - a.x + 1.f) * (a.w - a.y + 1.f); }

// The comparison  box_iou_plus1(a, b) >= thr  (ge) /  > thr  -- the same truth value as the rounded quotient gives, without
// the division in all but a sliver of cases.  r = fma(-thr, uni, inter) is (inter - thr uni) rounded once, so it carries the
// sign of (inter / uni - thr) whenever it is not zero.  The ROUNDED quotient can sit on the other side of thr than the real
// one only when the real one is within an ulp of thr, i.e. |inter - thr uni| < 2^-22 thr uni; inside 2^-21 thr uni (and for
// uni <= 0, NaNs, thr <= 0) the division is done as before.  aa / ab: box_area_plus1 of a / b (the same expressions
// box_iou_plus1 evaluates, so `uni` is the same float).
__device__ __forceinline__ bool box_iou_hits(const float4 a, const float aa, const float4 b, const float ab, const float thr,
                                             const float band_k, const int ge) {
  const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y), xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
  const float w = fmaxf(0.f, xx2 - xx1 + 1.f), h = fmaxf(0.f, yy2 - yy1 + 1.f);
  const float inter = w * h;
  const float uni = aa + ab - inter;
  const float r = __builtin_fmaf(-thr, uni, inter);
  const float band = band_k * uni;  // band_k = 2^-21 thr (<= 0 switches the shortcut off)
  if (band > 0.f && r > band) return true;
  if (band > 0.f && r < -band) return false;
  const float ovr = inter / uni;
  return ge ? (ovr >= thr) : (ovr > thr);
}
__device__ __forceinline__ float iou_band_k(float thr) { return thr > 0.f ? thr * 4.76837158203125e-07f : 0.f; }

}  // namespace hvr
