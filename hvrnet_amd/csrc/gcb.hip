// Global context block (GCNet), forward only.  Replaces mmdet/ops/context_block.py:64-104 (spatial_pool, the two bottleneck
// transforms, the fusion) and the residual add + ReLU that close the Bottleneck behind it (resnet.py:249-264).  The rule is
// stated in include/hvr_hip.h.  Three steps:
//   gcb_pool_kernel       ONE pass over the map u [B][P][C].  grid (S, B): the P pixels of a frame are cut into S runs of `chunk`
//                         pixels, one workgroup each.  A wave takes a pixel at a time: lane l holds the 16-byte channel pieces l,
//                         l + 64, ... of it, so the logit's dot product and the weighted sum use the same registers; the logit is a
//                         wave reduction (every lane ends with the same value).  Each wave keeps an online softmax state -- running
//                         maximum m, sum s, acc[C] rescaled when m grows --, the four waves of the workgroup are merged through LDS
//                         in a fixed order and ONE f32 partial (m, s, acc[C]) goes to the workspace slab.  No atomics: the result
//                         depends on the shape only, never on the schedule.
//   gcb_transform_kernel  one workgroup of 16 waves per frame and fusion branch: merges the S partials into ctx (maximum over the splits, rescale, divide), then
//                         per fusion branch W1 ctx + b1 (a wave per row), LayerNorm (biased variance, eps inside the root), ReLU,
//                         W2 g + b2 (a thread per channel on the TRANSPOSED W2, so the loads run along channels), sigmoid for mul.
//   gcb_apply_kernel      y = act(u * m[n][c] + t[n][c] (+ resid)), 16 bytes per lane, f32 math, one rounding; a lane reads its pieces
//                         of u and resid before it writes the same pieces of y, so y may be u or resid.
// The average pool is the same kernel without the logits (every weight 1).
#include "common.h"

namespace hvr {

constexpr int kGcbMaxC = 2048;
constexpr int kGcbSlabPad = 4;       // a partial is [m, s, 0, 0, acc[C]]: acc stays 16-byte aligned
constexpr int kGcbMaxSplits = 256;

// S and the pixels of a split, from the shape alone: at least 64 pixels per workgroup (16 per wave), about 1024 workgroups per call
void gcb_split(int B, int P, int* S, int* chunk) {
  long s = (P + 63) / 64;
  const long cap = 1024 / B > 1 ? 1024 / B : 1;
  if (s > cap) s = cap;
  if (s > kGcbMaxSplits) s = kGcbMaxSplits;
  if (s < 1) s = 1;
  const int ch = (int)((P + s - 1) / s);
  *chunk = ch;
  *S = (P + ch - 1) / ch;              // no empty split
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T> __device__ __forceinline__ void gcb_unpack(const uint4& r, float* f) {
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  } else {
    unpack2<T>(r.x, f[0], f[1]); unpack2<T>(r.y, f[2], f[3]); unpack2<T>(r.z, f[4], f[5]); unpack2<T>(r.w, f[6], f[7]);
  }
}
template <typename T> __device__ __forceinline__ uint4 gcb_pack(const float* f) {
  if constexpr (std::is_same<T, float>::value)
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  else
    return make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}

// NV: 16-byte pieces per lane (C / CV <= 64 * NV); PU: pixels a wave has in flight; ATT: attention pooling (else the mean)
template <typename T, int NV, int PU, bool ATT>
__global__ __launch_bounds__(256) void gcb_pool_kernel(const T* __restrict__ u, const float* __restrict__ wm, float* __restrict__ ws, int P, int C,
                                                       int S, int chunk) {
  constexpr int CV = 16 / (int)sizeof(T);
  __shared__ float sm[4], ss[4];
  __shared__ float sacc[4][kGcbMaxC];
  const int j = blockIdx.x, b = blockIdx.y;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int nvec = C / CV;
  const int p0 = j * chunk, p1 = min(P, p0 + chunk);          // p0 < P (no empty split)
  const T* ub = u + (long)b * P * C;

  float w[NV][CV];
  if constexpr (ATT) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = lane + 64 * i;
#pragma unroll
      for (int e = 0; e < CV; ++e) w[i][e] = v < nvec ? wm[v * CV + e] : 0.f;
    }
  }
  float acc[NV][CV];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < CV; ++e) acc[i][e] = 0.f;
  float m = -INFINITY, s = 0.f;

  // the pieces of PU pixels from p on (a pixel past the split's end repeats the last one: the address stays inside the map)
  auto load = [&](uint4 (&raw)[PU][NV], int p) {
#pragma unroll
    for (int q = 0; q < PU; ++q) {
      const T* row = ub + (long)min(p + q, p1 - 1) * C;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = lane + 64 * i;
        raw[q][i] = v < nvec ? *reinterpret_cast<const uint4*>(row + v * CV) : make_uint4(0, 0, 0, 0);
      }
    }
  };

  uint4 cur[PU][NV], nxt[PU][NV];
  int p = p0 + wave * PU;
  if (p < p1) load(cur, p);
  for (; p < p1; p += 4 * PU) {
    const int pn = p + 4 * PU;
    if (pn < p1) load(nxt, pn);
    float e[PU];
    if constexpr (ATT) {
      float l[PU];
      float mn = m;
#pragma unroll
      for (int q = 0; q < PU; ++q) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          float x[CV];
          gcb_unpack<T>(cur[q][i], x);
#pragma unroll
          for (int k = 0; k < CV; ++k) d += x[k] * w[i][k];
        }
        l[q] = p + q < p1 ? wave_sum(d) : -INFINITY;
        mn = fmaxf(mn, l[q]);
      }
      const float sc = m == -INFINITY ? 0.f : expf(m - mn);
      s *= sc;
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int k = 0; k < CV; ++k) acc[i][k] *= sc;
#pragma unroll
      for (int q = 0; q < PU; ++q) {
        e[q] = p + q < p1 ? expf(l[q] - mn) : 0.f;
        s += e[q];
      }
      m = mn;
    } else {
#pragma unroll
      for (int q = 0; q < PU; ++q) {
        e[q] = p + q < p1 ? 1.f : 0.f;
        s += e[q];
      }
      m = 0.f;
    }
#pragma unroll
    for (int q = 0; q < PU; ++q)
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float x[CV];
        gcb_unpack<T>(cur[q][i], x);
#pragma unroll
        for (int k = 0; k < CV; ++k) acc[i][k] += e[q] * x[k];
      }
#pragma unroll
    for (int q = 0; q < PU; ++q)
#pragma unroll
      for (int i = 0; i < NV; ++i) cur[q][i] = nxt[q][i];
  }

  // the four waves -> one partial, in wave order (a wave that saw no pixel has m = -inf, s = 0, acc = 0 and weighs 0)
  if (lane == 0) { sm[wave] = m; ss[wave] = s; }
  __syncthreads();
  const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  const float scw = m == -INFINITY ? 0.f : expf(m - M);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
#pragma unroll
      for (int k = 0; k < CV; ++k) sacc[wave][v * CV + k] = acc[i][k] * scw;
    }
  }
  __syncthreads();
  float* slab = ws + ((long)b * S + j) * (C + kGcbSlabPad);
  if (threadIdx.x == 0) {
    float st = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) st += sm[k] == -INFINITY ? 0.f : ss[k] * expf(sm[k] - M);
    slab[0] = M; slab[1] = st; slab[2] = 0.f; slab[3] = 0.f;
  }
  for (int c = (int)threadIdx.x; c < C; c += 256) slab[kGcbSlabPad + c] = ((sacc[0][c] + sacc[1][c]) + sacc[2][c]) + sacc[3][c];
}

template <typename T, int NV, int PU>
static hipError_t launch_gcb_pool_nv(const void* u, const float* wm, float* ws, int B, int P, int C, int S, int chunk, hipStream_t st) {
  if (wm)
    hipLaunchKernelGGL((gcb_pool_kernel<T, NV, PU, true>), dim3(S, B), dim3(256), 0, st, (const T*)u, wm, ws, P, C, S, chunk);
  else
    hipLaunchKernelGGL((gcb_pool_kernel<T, NV, PU, false>), dim3(S, B), dim3(256), 0, st, (const T*)u, wm, ws, P, C, S, chunk);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_gcb_pool(const void* u, const float* wm, float* ws, int B, int P, int C, int S, int chunk, hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int nv = (C / CV + 63) / 64;
  if (nv <= 1) return launch_gcb_pool_nv<T, 1, 4>(u, wm, ws, B, P, C, S, chunk, st);
  if (nv <= 2) return launch_gcb_pool_nv<T, 2, 2>(u, wm, ws, B, P, C, S, chunk, st);
  if (nv <= 4) return launch_gcb_pool_nv<T, 4, 1>(u, wm, ws, B, P, C, S, chunk, st);
  if constexpr (std::is_same<T, float>::value) {
    if (nv <= 8) return launch_gcb_pool_nv<T, 8, 1>(u, wm, ws, B, P, C, S, chunk, st);
  }
  return hipErrorInvalidValue;
}

// shapes are validated by the C ABI (capi.hip: hvr_gcb_pool)
hipError_t run_gcb_pool(const void* u, const float* wm, float* ws, int B, int P, int C, int dtype, hipStream_t st) {
  int S, chunk;
  gcb_split(B, P, &S, &chunk);
  if (dtype == DT_BF16) return launch_gcb_pool<bf16_t>(u, wm, ws, B, P, C, S, chunk, st);
  if (dtype == DT_F16) return launch_gcb_pool<f16_t>(u, wm, ws, B, P, C, S, chunk, st);
  if (dtype == DT_F32) return launch_gcb_pool<float>(u, wm, ws, B, P, C, S, chunk, st);
  return hipErrorInvalidValue;
}

// ---- transform
struct GcbMlp { const float *w1, *b1, *gamma, *beta, *w2t, *b2; };   // w1 [R][C], LayerNorm affine [R], w2t [R][C] (W2 transposed), b2 [C]

constexpr int kGcbTfThreads = 1024, kGcbTfWaves = kGcbTfThreads / 64;

// the sum of v over the threads of the workgroup, the same value in every thread (red: one float per wave), added in wave order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                       // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kGcbTfWaves; ++k) t += red[k];
  return t;
}

// grid (B, branches present): a workgroup of 16 waves merges the frame's partials (both workgroups of a frame compute the same ctx, in
// the same order) and runs ONE branch
__global__ __launch_bounds__(kGcbTfThreads) void gcb_transform_kernel(const float* __restrict__ ws, int C, int R, int S, GcbMlp mul, GcbMlp add,
                                                                      int has_mul, float* __restrict__ mo, float* __restrict__ to) {
  __shared__ float ctx[kGcbMaxC];
  __shared__ float hid[kGcbMaxC];
  __shared__ float scale[kGcbMaxSplits];
  __shared__ float red[kGcbTfWaves];
  const int b = blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool is_mul = has_mul && blockIdx.y == 0;
  const float* slabs = ws + (long)b * S * (C + kGcbSlabPad);
  const long ld = C + kGcbSlabPad;
  // the frame maximum, then every split's weight against it (a split far below underflows to exactly 0)
  float M = -INFINITY;
  for (int j = lane; j < S; j += 64) M = fmaxf(M, slabs[j * ld]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
  for (int j = tid; j < S; j += kGcbTfThreads) scale[j] = expf(slabs[j * ld] - M);
  __syncthreads();
  float den = 0.f;
  for (int j = 0; j < S; ++j) den += slabs[j * ld + 1] * scale[j];
  for (int c = tid; c < C; c += kGcbTfThreads) {
    float a = 0.f;
#pragma unroll 8
    for (int j = 0; j < S; ++j) a += slabs[j * ld + kGcbSlabPad + c] * scale[j];
    ctx[c] = a / den;
  }
  __syncthreads();
  const GcbMlp w = is_mul ? mul : add;
  float* dst = (is_mul ? mo : to) + (long)b * C;
  // W1 ctx + b1: a wave takes four rows at a time (their loads in flight together), 16 bytes per lane along C (C % 64 == 0)
  for (int r0 = wave * 4; r0 < R; r0 += kGcbTfWaves * 4) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 4; c < C; c += 256) {
      float4 a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const float4*>(w.w1 + (long)min(r0 + k, R - 1) * C + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] += a[k].x * ctx[c] + a[k].y * ctx[c + 1] + a[k].z * ctx[c + 2] + a[k].w * ctx[c + 3];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = wave_sum(d[k]);
      if (lane == 0 && r0 + k < R) hid[r0 + k] = v + w.b1[r0 + k];
    }
  }
  __syncthreads();
  // LayerNorm over the R values: biased variance, eps inside the root
  float part = 0.f;
  for (int r = tid; r < R; r += kGcbTfThreads) part += hid[r];
  const float mean = block_sum(part, red) / (float)R;
  part = 0.f;
  for (int r = tid; r < R; r += kGcbTfThreads) { const float dlt = hid[r] - mean; part += dlt * dlt; }
  const float var = block_sum(part, red) / (float)R;
  const float rstd = 1.f / sqrtf(var + 1e-5f);
  __syncthreads();
  for (int r = tid; r < R; r += kGcbTfThreads) hid[r] = fmaxf((hid[r] - mean) * rstd * w.gamma[r] + w.beta[r], 0.f);
  __syncthreads();
  // W2 g + b2: a thread per channel on the transposed W2 (the loads of a row run along channels), rows in order
  for (int c = tid; c < C; c += kGcbTfThreads) {
    float a = 0.f;
#pragma unroll 8
    for (int r = 0; r < R; ++r) a += w.w2t[(long)r * C + c] * hid[r];
    a += w.b2[c];
    dst[c] = is_mul ? 1.f / (1.f + expf(-a)) : a;
  }
}

// R <= kGcbMaxC (R = int(C * ratio), ratio <= 1) is validated by the C ABI
hipError_t run_gcb_transform(const float* ws, int B, int P, int C, int R, const float* const* mul, const float* const* add, float* mo, float* to,
                             hipStream_t st) {
  int S, chunk;
  gcb_split(B, P, &S, &chunk);
  GcbMlp a = {}, b = {};
  if (mul) a = GcbMlp{mul[0], mul[1], mul[2], mul[3], mul[4], mul[5]};
  if (add) b = GcbMlp{add[0], add[1], add[2], add[3], add[4], add[5]};
  hipLaunchKernelGGL(gcb_transform_kernel, dim3(B, (mul ? 1 : 0) + (add ? 1 : 0)), dim3(kGcbTfThreads), 0, st, ws, C, R, S, a, b, mul ? 1 : 0, mo, to);
  return hipGetLastError();
}

// ---- apply
// grid (pixel tiles, B).  A lane keeps ONE 16-byte channel piece: it loads that piece of m and t once and walks down the pixels of its
// tile, four loads of u (and of resid) in flight; the workgroup's 256 lanes are rows x (C / CV) pieces.
constexpr int kGcbApplyIters = 16;       // pixels per lane

template <typename T>
__global__ __launch_bounds__(256) void gcb_apply_kernel(const T* u, const float* __restrict__ mo, const float* __restrict__ to, const T* resid, T* y,
                                                        int P, int C, int relu) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int vpp = C / CV;                                   // pieces per pixel
  const int lanes_c = vpp < 256 ? vpp : 256;
  const int rows = 256 / lanes_c;
  const int row = (int)threadIdx.x / lanes_c, cl = (int)threadIdx.x - row * lanes_c;
  if (row >= rows) return;
  const int n = blockIdx.y;
  const int pix0 = blockIdx.x * (rows * kGcbApplyIters), pix1 = min(P, pix0 + rows * kGcbApplyIters);
  const long frame = (long)n * P * C;
  for (int cv = cl; cv < vpp; cv += lanes_c) {
    const int c = cv * CV;
    float mm[CV], tt[CV];
#pragma unroll
    for (int k = 0; k < CV; k += 4) {
      const float4 a = mo ? *reinterpret_cast<const float4*>(mo + (long)n * C + c + k) : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 b = to ? *reinterpret_cast<const float4*>(to + (long)n * C + c + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      mm[k] = a.x; mm[k + 1] = a.y; mm[k + 2] = a.z; mm[k + 3] = a.w;
      tt[k] = b.x; tt[k + 1] = b.y; tt[k + 2] = b.z; tt[k + 3] = b.w;
    }
    for (int p = pix0 + row; p < pix1; p += 4 * rows) {
      uint4 xr[4], rr[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long off = frame + (long)min(p + q * rows, pix1 - 1) * C + c;   // (past the tile's end: the last pixel again, not stored)
        xr[q] = *reinterpret_cast<const uint4*>(u + off);
        if (resid) rr[q] = *reinterpret_cast<const uint4*>(resid + off);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (p + q * rows >= pix1) break;
        float x[CV], r[CV];
        gcb_unpack<T>(xr[q], x);
        if (resid) gcb_unpack<T>(rr[q], r);
#pragma unroll
        for (int k = 0; k < CV; ++k) {
          float v = x[k];
          if (mo) v = v * mm[k];
          if (to) v = v + tt[k];
          if (resid) v = v + r[k];
          x[k] = relu ? fmaxf(v, 0.f) : v;
        }
        *reinterpret_cast<uint4*>(y + frame + (long)(p + q * rows) * C + c) = gcb_pack<T>(x);
      }
    }
  }
}

template <typename T>
static hipError_t launch_gcb_apply(const void* u, const float* mo, const float* to, const void* resid, void* y, int B, int P, int C, int relu,
                                   hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int vpp = C / CV, rows = 256 / (vpp < 256 ? vpp : 256);
  const int tiles = (P + rows * kGcbApplyIters - 1) / (rows * kGcbApplyIters);
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gcb_apply_kernel<T>), dim3(tiles, B), dim3(256), 0, st, (const T*)u, mo, to, (const T*)resid, (T*)y, P, C, relu);
  return hipGetLastError();
}

hipError_t run_gcb_apply(const void* u, const float* mo, const float* to, const void* resid, void* y, int B, int P, int C, int relu, int dtype,
                         hipStream_t st) {
  if (dtype == DT_BF16) return launch_gcb_apply<bf16_t>(u, mo, to, resid, y, B, P, C, relu, st);
  if (dtype == DT_F16) return launch_gcb_apply<f16_t>(u, mo, to, resid, y, B, P, C, relu, st);
  if (dtype == DT_F32) return launch_gcb_apply<float>(u, mo, to, resid, y, B, P, C, relu, st);
  return hipErrorInvalidValue;
}

}  // namespace hvr
