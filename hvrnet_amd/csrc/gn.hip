// Group normalisation, forward only (torch.nn.GroupNorm at inference: no running statistics, so every map is reduced per frame and
// group and then rescaled).  The rule is stated in include/hvr_hip.h.  Two launches per norm:
//   gn_stats_kernel   ONE pass over the map u [B][P][C].  grid (S, B): the P pixels of a frame are cut into S runs of `chunk` pixels, one
//                     workgroup of four waves each.  A wave covers 64 / LC pixels at a time, LC = min(64, the pieces of a pixel rounded up to
//                     a power of two) lanes per pixel; lane l holds the 16-byte channel pieces l, l + 64, ... of its pixel and walks down
//                     the run, the loads of the next step in flight while this one is reduced (register double buffer).  Every piece is
//                     reduced to a centred partial (mean, M2) per group it touches and merged into the lane's running partial by Chan's
//                     formula; the lanes of a group (its pieces, then the pixel rows of the wave) are merged by xor shuffles, the lower
//                     lane as the left operand; the four waves through LDS in wave order; ONE f32 partial (count, mean - pivot, M2, pivot) per group
//                     goes to the workspace.  No atomics, no sum of squares: the result depends on the shape only.  Every value is taken
//                     relative to the group's pivot (its first channel at the frame's first pixel), which rides in the partial's fourth
//                     slot: the partial means are (mean - pivot) and never carry the mean's magnitude.
//   gn_apply_kernel   grid (pixel tiles, B).  Every workgroup first merges the S partials of its frame's groups, in run order, into
//                     pivot[G], (mean - pivot)[G] and rstd[G] in LDS (and those of the residual's workspace when the shortcut is normalised in the same pass);
//                     a lane keeps ONE 16-byte channel piece, forms a = rstd * gamma for its channels once, and walks down the pixels of
//                     its tile: y = act(((u - pivot) - (mean - pivot)) * a + beta (+ r)), 16 bytes per lane, f32 math, one rounding.  A lane reads its pieces
//                     of u and resid before it writes the same pieces of y, so y may be u or resid.
#include "common.h"

namespace hvr {

constexpr int kGnMaxC = 2048;
constexpr int kGnMaxG = kGnMaxC / 2;     // Cg >= 2
constexpr int kGnMaxSplits = 64;

// S and the pixels of a run, from the shape alone: at least 64 pixels per workgroup, about 1024 workgroups per call, at most 64 runs (every
// workgroup of the apply merges all S partials of its frame)
void gn_split(int B, int P, int* S, int* chunk) {
  long s = (P + 63) / 64;
  const long cap = 1024 / B > 1 ? 1024 / B : 1;
  if (s > cap) s = cap;
  if (s > kGnMaxSplits) s = kGnMaxSplits;
  if (s < 1) s = 1;
  const int ch = (int)((P + s - 1) / s);
  *chunk = ch;
  *S = (P + ch - 1) / ch;              // no empty run
}

template <typename T> __device__ __forceinline__ void gn_unpack(const uint4& r, float* f) {
  if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
  } else {
    unpack2<T>(r.x, f[0], f[1]); unpack2<T>(r.y, f[2], f[3]); unpack2<T>(r.z, f[4], f[5]); unpack2<T>(r.w, f[6], f[7]);
  }
}
template <typename T> __device__ __forceinline__ uint4 gn_pack(const float* f) {
  if constexpr (std::is_same<T, float>::value)
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  else
    return make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}

// one stored element as f32
template <typename T> __device__ __forceinline__ float gn_elem(const T* p) {
  if constexpr (std::is_same<T, float>::value) {
    return *p;
  } else {
    float lo, hi;
    unpack2<T>((uint32_t)*p, lo, hi);
    return lo;
  }
}

// Chan's merge of the centred partials a = (na, ma, qa) and b = (nb, mb, qb), given nb / n and na * nb / n (0 when n = 0: an empty
// partial merges to the other one exactly)
__device__ __forceinline__ void gn_merge(float ma, float qa, float mb, float qb, float wb, float wab, float& m, float& q) {
  const float d = mb - ma;
  m = ma + d * wb;
  q = (qa + qb) + d * d * wab;
}

// NV: 16-byte pieces per lane; GP: groups inside one piece (1 when a group is at least a piece wide); PU: pixels a lane has in flight
// beside the ones it reduces
template <typename T, int NV, int GP, int PU>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ u, float* __restrict__ ws, int P, int C, int G, int S, int chunk,
                                                       int lc_log2) {
  constexpr int CV = 16 / (int)sizeof(T);
  constexpr int E = CV / GP;                                  // elements of one group inside a piece
  __shared__ float sn[4];
  __shared__ float smean[4][kGnMaxG], sm2[4][kGnMaxG];
  const int j = blockIdx.x, b = blockIdx.y;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int LC = 1 << lc_log2, rows_w = 64 >> lc_log2;        // lanes per pixel, pixels per wave
  const int cl = lane & (LC - 1), row = wave * rows_w + (lane >> lc_log2), R = 4 * rows_w;
  const int nvec = C / CV, Cg = C / G;
  const int ppg = GP > 1 ? 1 : Cg / CV;                       // pieces per group
  const int p0 = j * chunk, p1 = min(P, p0 + chunk);          // p0 < P (no empty run)
  const T* ub = u + (long)b * P * C;

  // the pivot of a group: its first channel at the frame's first pixel.  Every value is taken relative to it (an exact subtraction
  // where the group's spread is small against its mean), so no partial mean ever carries the mean's magnitude.
  float n = 0.f, mean[NV][GP], m2[NV][GP], piv[NV][GP];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < GP; ++k) {
      mean[i][k] = m2[i][k] = 0.f;
      const int v = cl + 64 * i;
      piv[i][k] = v < nvec ? gn_elem<T>(ub + (GP > 1 ? v * GP + k : v / ppg) * Cg) : 0.f;
    }

  // the pieces of the PU pixels p, p + R, ... (a pixel past the run's end repeats the last one: the address stays inside the map)
  auto load = [&](uint4 (&raw)[PU][NV], int p) {
#pragma unroll
    for (int q = 0; q < PU; ++q) {
      const T* px = ub + (long)min(p + q * R, p1 - 1) * C;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = cl + 64 * i;
        raw[q][i] = v < nvec ? *reinterpret_cast<const uint4*>(px + v * CV) : make_uint4(0, 0, 0, 0);
      }
    }
  };

  uint4 cur[PU][NV], nxt[PU][NV];
  int p = p0 + row;
  if (p < p1) load(cur, p);
  for (; p < p1; p += R * PU) {
    const int pn = p + R * PU;
    if (pn < p1) load(nxt, pn);
#pragma unroll
    for (int q = 0; q < PU; ++q) {
      if (p + q * R < p1) {
        const float nt = n + (float)E;
        const float wb = (float)E / nt, wab = n * wb;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          float x[CV];
          gn_unpack<T>(cur[q][i], x);
#pragma unroll
          for (int k = 0; k < GP; ++k) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) { x[k * E + e] -= piv[i][k]; s += x[k * E + e]; }
            const float mb = s * (1.f / (float)E);
            float qb = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) { const float d = x[k * E + e] - mb; qb += d * d; }
            gn_merge(mean[i][k], m2[i][k], mb, qb, wb, wab, mean[i][k], m2[i][k]);
          }
        }
        n = nt;
      }
    }
#pragma unroll
    for (int q = 0; q < PU; ++q)
#pragma unroll
      for (int i = 0; i < NV; ++i) cur[q][i] = nxt[q][i];
  }

  // lanes of one group inside the wave: its pieces of a pixel (offsets 1 .. ppg / 2), then the pixel rows (offsets LC .. 32).  Both lanes
  // of a pair compute merge(lower lane, upper lane): the same bits in both.
  auto merge_lanes = [&](int off) {
    const float no = __shfl_xor(n, off, 64);
    const bool low = (lane & off) == 0;
    const float na = low ? n : no, nb = low ? no : n, nt = na + nb;
    const float wb = nt > 0.f ? nb / nt : 0.f, wab = na * wb;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < GP; ++k) {
        const float mo = __shfl_xor(mean[i][k], off, 64), qo = __shfl_xor(m2[i][k], off, 64);
        const float ma = low ? mean[i][k] : mo, mb = low ? mo : mean[i][k];
        const float qa = low ? m2[i][k] : qo, qb = low ? qo : m2[i][k];
        gn_merge(ma, qa, mb, qb, wb, wab, mean[i][k], m2[i][k]);
      }
    n = nt;
  };
  for (int off = 1; off < ppg; off <<= 1) merge_lanes(off);
  for (int off = LC; off < 64; off <<= 1) merge_lanes(off);

  // the four waves -> one partial per group, in wave order
  if (lane == 0) sn[wave] = n;
  if (lane < LC && (cl & (ppg - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = cl + 64 * i;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < GP; ++k) {
          const int g = GP > 1 ? v * GP + k : v / ppg;
          smean[wave][g] = mean[i][k];
          sm2[wave][g] = m2[i][k];
        }
      }
    }
  }
  __syncthreads();
  float4* out = reinterpret_cast<float4*>(ws) + ((long)b * S + j) * G;
  for (int g = (int)threadIdx.x; g < G; g += 256) {
    float na = sn[0], m = smean[0][g], q = sm2[0][g];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float nb = sn[w], nt = na + nb;
      const float wb = nt > 0.f ? nb / nt : 0.f;
      gn_merge(m, q, smean[w][g], sm2[w][g], wb, na * wb, m, q);
      na = nt;
    }
    out[g] = make_float4(na, m, q, gn_elem<T>(ub + g * Cg));
  }
}

template <typename T, int NV, int GP, int PU>
static hipError_t launch_gn_stats_i(const void* u, float* ws, int B, int P, int C, int G, int S, int chunk, hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int nvec = C / CV;
  int lc_log2 = 3;                                            // (nvec >= 8: C >= 64)
  while ((1 << lc_log2) < nvec && lc_log2 < 6) ++lc_log2;
  hipLaunchKernelGGL((gn_stats_kernel<T, NV, GP, PU>), dim3(S, B), dim3(256), 0, st, (const T*)u, ws, P, C, G, S, chunk, lc_log2);
  return hipGetLastError();
}

template <typename T, int GP>
static hipError_t launch_gn_stats_gp(const void* u, float* ws, int B, int P, int C, int G, int S, int chunk, hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int nv = (C / CV + 63) / 64;
  if (nv <= 1) return launch_gn_stats_i<T, 1, GP, 4>(u, ws, B, P, C, G, S, chunk, st);
  if (nv <= 2) return launch_gn_stats_i<T, 2, GP, 2>(u, ws, B, P, C, G, S, chunk, st);
  if (nv <= 4) return launch_gn_stats_i<T, 4, GP, 1>(u, ws, B, P, C, G, S, chunk, st);
  if constexpr (std::is_same<T, float>::value) {
    if (nv <= 8) return launch_gn_stats_i<T, 8, GP, 1>(u, ws, B, P, C, G, S, chunk, st);
  }
  return hipErrorInvalidValue;
}

template <typename T>
static hipError_t launch_gn_stats(const void* u, float* ws, int B, int P, int C, int G, int S, int chunk, hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int Cg = C / G;
  if (Cg >= CV) return launch_gn_stats_gp<T, 1>(u, ws, B, P, C, G, S, chunk, st);
  if (Cg * 2 == CV) return launch_gn_stats_gp<T, 2>(u, ws, B, P, C, G, S, chunk, st);
  if constexpr (CV == 8) {
    if (Cg * 4 == CV) return launch_gn_stats_gp<T, 4>(u, ws, B, P, C, G, S, chunk, st);
  }
  return hipErrorInvalidValue;
}

// shapes are validated by the C ABI (capi.hip: hvr_gn_stats)
hipError_t run_gn_stats(const void* u, float* ws, int B, int P, int C, int G, int dtype, hipStream_t st) {
  int S, chunk;
  gn_split(B, P, &S, &chunk);
  if (B > 65535) return hipErrorInvalidValue;
  if (dtype == DT_BF16) return launch_gn_stats<bf16_t>(u, ws, B, P, C, G, S, chunk, st);
  if (dtype == DT_F16) return launch_gn_stats<f16_t>(u, ws, B, P, C, G, S, chunk, st);
  if (dtype == DT_F32) return launch_gn_stats<float>(u, ws, B, P, C, G, S, chunk, st);
  return hipErrorInvalidValue;
}

// ---- apply
constexpr int kGnApplyIters = 32;        // pixels per lane: a workgroup streams 256 lanes x 16 bytes x 32 = 128 KB of u

// the S partials of group g of one frame, merged in run order -> (pivot, mean - pivot, rstd)
__device__ __forceinline__ void gn_merge_runs(const float4* __restrict__ part, int S, int G, int g, float eps, float& piv, float& mean, float& rstd) {
  const float4 a = part[g];
  float na = a.x, m = a.y, q = a.z;
  for (int s0 = 1; s0 < S; s0 += 8) {                       // eight partials in flight, merged in run order
    float4 c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = part[(long)min(s0 + k, S - 1) * G + g];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (s0 + k < S) {
        const float nt = na + c[k].x;
        const float wb = nt > 0.f ? c[k].x / nt : 0.f;
        gn_merge(m, q, c[k].y, c[k].z, wb, na * wb, m, q);
        na = nt;
      }
    }
  }
  piv = a.w;
  mean = m;
  rstd = 1.f / sqrtf(q / na + eps);
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* u, const float* __restrict__ ws, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, const T* resid, const float* __restrict__ ws_r,
                                                       const float* __restrict__ gamma_r, const float* __restrict__ beta_r, T* y, int P, int C,
                                                       int G, int S, int relu) {
  constexpr int CV = 16 / (int)sizeof(T);
  __shared__ float spiv[2][kGnMaxG], smean[2][kGnMaxG], srstd[2][kGnMaxG];
  const int n = blockIdx.y, Cg = C / G;
  for (int g = (int)threadIdx.x; g < G; g += 256) {
    gn_merge_runs(reinterpret_cast<const float4*>(ws) + (long)n * S * G, S, G, g, eps, spiv[0][g], smean[0][g], srstd[0][g]);
    if (ws_r) gn_merge_runs(reinterpret_cast<const float4*>(ws_r) + (long)n * S * G, S, G, g, eps, spiv[1][g], smean[1][g], srstd[1][g]);
  }
  __syncthreads();
  const int vpp = C / CV;                                   // pieces per pixel
  const int lanes_c = vpp < 256 ? vpp : 256;
  const int rows = 256 / lanes_c;
  const int row = (int)threadIdx.x / lanes_c, cl = (int)threadIdx.x - row * lanes_c;
  if (row >= rows) return;
  const int pix0 = blockIdx.x * (rows * kGnApplyIters), pix1 = min(P, pix0 + rows * kGnApplyIters);
  const long frame = (long)n * P * C;
  for (int cv = cl; cv < vpp; cv += lanes_c) {
    const int c = cv * CV;
    float kk[CV], mm[CV], aa[CV], bb[CV], kr[CV], mr[CV], ar[CV], br[CV];
#pragma unroll
    for (int k = 0; k < CV; ++k) {
      const int g = (c + k) / Cg;
      kk[k] = spiv[0][g];
      mm[k] = smean[0][g];
      aa[k] = srstd[0][g] * gamma[c + k];
      bb[k] = beta[c + k];
      if (ws_r) {
        kr[k] = spiv[1][g];
        mr[k] = smean[1][g];
        ar[k] = srstd[1][g] * gamma_r[c + k];
        br[k] = beta_r[c + k];
      }
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
        gn_unpack<T>(xr[q], x);
        if (resid) gn_unpack<T>(rr[q], r);
#pragma unroll
        for (int k = 0; k < CV; ++k) {
          float v = ((x[k] - kk[k]) - mm[k]) * aa[k] + bb[k];           // u - mean, the mean held as pivot + (mean - pivot)
          if (resid) v = v + (ws_r ? ((r[k] - kr[k]) - mr[k]) * ar[k] + br[k] : r[k]);
          x[k] = relu ? fmaxf(v, 0.f) : v;
        }
        *reinterpret_cast<uint4*>(y + frame + (long)(p + q * rows) * C + c) = gn_pack<T>(x);
      }
    }
  }
}

template <typename T>
static hipError_t launch_gn_apply(const void* u, const float* ws, const float* gamma, const float* beta, float eps, const void* resid,
                                  const float* ws_r, const float* gamma_r, const float* beta_r, void* y, int B, int P, int C, int G, int S, int relu,
                                  hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const int vpp = C / CV, rows = 256 / (vpp < 256 ? vpp : 256);
  const int tiles = (P + rows * kGnApplyIters - 1) / (rows * kGnApplyIters);
  if (B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gn_apply_kernel<T>), dim3(tiles, B), dim3(256), 0, st, (const T*)u, ws, gamma, beta, eps, (const T*)resid, ws_r, gamma_r, beta_r,
                     (T*)y, P, C, G, S, relu);
  return hipGetLastError();
}

hipError_t run_gn_apply(const void* u, const float* ws, const float* gamma, const float* beta, float eps, const void* resid, const float* ws_r,
                        const float* gamma_r, const float* beta_r, void* y, int B, int P, int C, int G, int relu, int dtype, hipStream_t st) {
  int S, chunk;
  gn_split(B, P, &S, &chunk);
  if (dtype == DT_BF16) return launch_gn_apply<bf16_t>(u, ws, gamma, beta, eps, resid, ws_r, gamma_r, beta_r, y, B, P, C, G, S, relu, st);
  if (dtype == DT_F16) return launch_gn_apply<f16_t>(u, ws, gamma, beta, eps, resid, ws_r, gamma_r, beta_r, y, B, P, C, G, S, relu, st);
  if (dtype == DT_F32) return launch_gn_apply<float>(u, ws, gamma, beta, eps, resid, ws_r, gamma_r, beta_r, y, B, P, C, G, S, relu, st);
  return hipErrorInvalidValue;
}

}  // namespace hvr
