// Sigmoid focal loss for gfx950 (mmdet/ops/sigmoid_focal_loss, losses/focal_loss.py; the rule: include/hvr_hip.h "Sigmoid focal loss").
// Built with -ffp-contract=off: tests/focal_refs.py bounds every product and sum as a rounding of its own.
//   focal_elem_kernel      loss [N][C] or d_logits [N][C] = dl/dx * d_loss from logits [N][ldl] (f32 / bf16 / half), f32 math.
//   focal_fused_kernel     the reduced form in ONE pass over f32 logits: d_logits [N][ldl] (pitch columns zero) and one f32 partial of
//                          sum w l per workgroup; focal_merge_kernel adds the partials in workgroup order and scales.  No atomics: the
//                          result depends on the shape only.
//   rpn_focal_loss_kernel  rpn_loss_kernel (targets.hip) with the focal rule at C = 1 in place of the BCE and both terms over the
//                          positive count; the smooth-L1 element is the shared one (smooth_l1_dev.h).
// Row mapping of the first two: G lanes share a row (G = the row's 16-byte pieces, or its elements when the pitch or an address
// rules 16-byte accesses out), 256 / G rows per workgroup step; a lane loads its row's target once and walks the row's columns.
#include "common.h"
#include "smooth_l1_dev.h"

namespace hvr {

constexpr int kFocalThreads = 256;
constexpr int kFocalElemsPerWg = 2048;    // N * C elements a workgroup of the reduced form takes, at least
constexpr int kFocalMaxSplits = 2048;

// S workgroups of `rows` rows each (the last may hold fewer, none is empty), from the shape alone
void focal_split(int N, int C, int* S, int* rows) {
  long s = ((long)N * C + kFocalElemsPerWg - 1) / kFocalElemsPerWg;
  if (s > kFocalMaxSplits) s = kFocalMaxSplits;
  if (s > N) s = N;
  if (s < 1) s = 1;
  const int r = (int)((N + s - 1) / s);
  *rows = r;
  *S = (N + r - 1) / r;
}

namespace {

struct FocalTerm { float l, g; };

// one element of the rule: loss l and dl/dx at logit x, for a positive (t == c + 1) or a negative column
__device__ __forceinline__ FocalTerm focal_term(float x, bool positive, float gamma, float alpha, float one_m_alpha) {
  const float e = expf(-fabsf(x));
  const float L = log1pf(e);
  const float lp = fminf(x, 0.f) - L;          // log p
  const float lq = -fmaxf(x, 0.f) - L;         // log (1 - p)
  const float r = 1.f / (1.f + e), er = e * r;
  const float p = x >= 0.f ? r : er, q = x >= 0.f ? er : r;     // p = sigmoid(x), q = 1 - p = sigmoid(-x)
  FocalTerm t;
  if (positive) {
    const float c = alpha * expf(gamma * lq);                    // alpha (1 - p)^gamma
    t.l = c * -lp;
    t.g = -(c * (q - gamma * p * lp));
  } else {
    const float c = one_m_alpha * expf(gamma * lp);              // (1 - alpha) p^gamma
    t.l = c * -lq;
    t.g = c * (p - gamma * q * lq);
  }
  return t;
}

template <typename T, int V> __device__ __forceinline__ void focal_load(const T* p, float (&v)[V]) {
  if constexpr (V == 1) {
    v[0] = ElemTraits<T>::load(p);
  } else {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    if constexpr (std::is_same<T, float>::value) {
      v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y); v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
    } else {
      unpack2<T>(r.x, v[0], v[1]); unpack2<T>(r.y, v[2], v[3]); unpack2<T>(r.z, v[4], v[5]); unpack2<T>(r.w, v[6], v[7]);
    }
  }
}

}  // namespace

// V elements per lane and step: 16 bytes (4 f32, 8 bf16 / half) or 1.  BWD: out = dl/dx * d_loss, else out = l.
template <typename T, int V, bool BWD>
__global__ __launch_bounds__(kFocalThreads) void focal_elem_kernel(const T* __restrict__ x, int ldl, const long long* __restrict__ tgt,
                                                                   const float* __restrict__ d_loss, int N, int C, float gamma, float alpha,
                                                                   float* __restrict__ out, int G, int R) {
  const int rib = (int)threadIdx.x / G, sub = (int)threadIdx.x - rib * G;
  const long n = (long)blockIdx.x * R + rib;
  if (rib >= R || n >= N) return;
  const long long t = tgt[n];
  const float oma = 1.f - alpha;
  const T* row = x + n * ldl;
  float* orow = out + n * C;
  const float* grow = BWD ? d_loss + n * C : nullptr;
  for (int c0 = sub * V; c0 < C; c0 += G * V) {
    float v[V], o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = 0.f;
    if (t >= 0) {
      focal_load<T, V>(row + c0, v);
#pragma unroll
      for (int k4 = 0; k4 < V; k4 += 4) {
        float dl[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (V == 1) {
          if (BWD) dl[0] = grow[c0];
        } else if (BWD) {
          if (c0 + k4 < C) {
            const float4 d4 = *reinterpret_cast<const float4*>(grow + c0 + k4);
            dl[0] = d4.x; dl[1] = d4.y; dl[2] = d4.z; dl[3] = d4.w;
          }
        }
#pragma unroll
        for (int k = k4; k < (V == 1 ? 1 : k4 + 4); ++k) {
          const int c = c0 + k;
          if (c < C) {
            const FocalTerm f = focal_term(v[k], t == c + 1, gamma, alpha, oma);
            o[k] = BWD ? f.g * dl[k - k4] : f.l;
          }
        }
      }
    }
    if constexpr (V == 1) {
      orow[c0] = o[0];
    } else {
#pragma unroll
      for (int k4 = 0; k4 < V; k4 += 4)     // C is a multiple of 4 here: a group of four is inside the row or outside it
        if (c0 + k4 < C) *reinterpret_cast<float4*>(orow + c0 + k4) = make_float4(o[k4], o[k4 + 1], o[k4 + 2], o[k4 + 3]);
    }
  }
}

// workgroup b takes rows [b rpw, min(N, (b + 1) rpw)); partial[b] = sum over its rows of w[n] sum_c l[n][c], added per lane in row-then-column
// order, then over the wave by xor shuffles, then over the four waves in wave order
template <int V>
__global__ __launch_bounds__(kFocalThreads) void focal_fused_kernel(const float* __restrict__ x, int ldl, const long long* __restrict__ tgt,
                                                                    const float* __restrict__ w, int N, int C, float gamma, float alpha,
                                                                    float loss_weight, float avg_host, const int* __restrict__ counts,
                                                                    float* __restrict__ partial, float* __restrict__ d, int G, int R, int rpw) {
  __shared__ float red[kFocalThreads / 64];
  const int tid = (int)threadIdx.x, rib = tid / G, sub = tid - rib * G;
  const float avg = counts ? (float)max(counts[0], 1) : avg_host;
  const float scale = loss_weight / avg, oma = 1.f - alpha;
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < (long)N ? r0 + rpw : (long)N;
  float acc = 0.f;
  if (rib < R) {
    for (long n = r0 + rib; n < r1; n += R) {
      const long long t = tgt[n];
      const float wn = w ? w[n] : 1.f, coef = scale * wn;
      const float* row = x + n * ldl;
      float* drow = d + n * ldl;
      for (int c0 = sub * V; c0 < ldl; c0 += G * V) {
        float v[V], o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = 0.f;
        if (t >= 0 && c0 < C) {
          focal_load<float, V>(row + c0, v);
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const int c = c0 + k;
            if (c < C) {
              const FocalTerm f = focal_term(v[k], t == c + 1, gamma, alpha, oma);
              acc += wn * f.l;
              o[k] = coef * f.g;
            }
          }
        }
        if constexpr (V == 1)
          drow[c0] = o[0];
        else
          *reinterpret_cast<float4*>(drow + c0) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave: lane i adds partials i, i + 64, ... in that order, xor shuffles, out1 = sum * (loss_weight / avg)
__global__ __launch_bounds__(64) void focal_merge_kernel(const float* __restrict__ partial, int S, float loss_weight, float avg_host,
                                                         const int* __restrict__ counts, float* __restrict__ out1) {
  const float avg = counts ? (float)max(counts[0], 1) : avg_host;
  float s = 0.f;
  for (int j = (int)threadIdx.x; j < S; j += 64) s += partial[j];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) out1[0] = s * (loss_weight / avg);
}

// One workgroup, fixed order, as rpn_loss_kernel.  avg = max(counts[0], 1) for BOTH terms (anchor_head.py:194-195).
__global__ __launch_bounds__(1024) void rpn_focal_loss_kernel(const float* __restrict__ o, int ldo, int A, int rows,
                                                              const long long* __restrict__ labels, const float* __restrict__ label_w,
                                                              const float* __restrict__ bbox_t, const float* __restrict__ bbox_w,
                                                              const int* __restrict__ counts, float beta, float gamma, float alpha,
                                                              float w_cls, float w_bbox, float* __restrict__ out2, float* __restrict__ d_o) {
  __shared__ float red[2][1024];
  const int tid = threadIdx.x;
  const float avg = (float)max(counts[0], 1);
  const float sc = w_cls / avg, oma = 1.f - alpha;
  const int M = rows * A;
  float lc = 0.f, lb = 0.f;
  for (int m = tid; m < M; m += 1024) {
    const int r = m / A, a = m - r * A;
    const float* row = o + (long)r * ldo;
    float* drow = d_o + (long)r * ldo;
    if (a == 0)   // columns 5A .. ldo belong to no anchor: their gradient is zero (d_o arrives uninitialised)
      for (int c = 5 * A; c < ldo; ++c) drow[c] = 0.f;
    const long long t = labels[m];
    const float w = label_w[m];
    float gx = 0.f;
    if (t >= 0) {
      const FocalTerm f = focal_term(row[a], t == 1, gamma, alpha, oma);
      lc += w * f.l;
      gx = sc * w * f.g;
    }
    drow[a] = gx;
    for (int e = 0; e < 4; ++e) {
      float g;
      lb += smooth_l1_term(row[A + a * 4 + e] - bbox_t[(long)m * 4 + e], beta, bbox_w[(long)m * 4 + e], avg, &g);
      drow[A + a * 4 + e] = w_bbox * g;
    }
  }
  red[0][tid] = lc; red[1][tid] = lb;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { out2[0] = red[0][0] * sc; out2[1] = red[1][0] / avg * w_bbox; }
}

namespace {

inline bool is16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lanes per row and rows per workgroup step for rows of `cols` columns taken V at a time
inline void focal_map(int cols, int V, int* G, int* R) {
  int g = (cols + V - 1) / V;
  if (g > kFocalThreads) g = kFocalThreads;
  *G = g;
  *R = kFocalThreads / g;
}

template <typename T, bool BWD>
hipError_t launch_elem(const void* x, int ldl, const long long* t, const float* d_loss, int N, int C, float gamma, float alpha, float* out,
                       hipStream_t s) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool wide = ldl % VW == 0 && C % 4 == 0 && is16(x) && is16(out) && (!BWD || is16(d_loss));
  int G, R;
  focal_map(C, wide ? VW : 1, &G, &R);
  const dim3 grid((unsigned)(((long)N + R - 1) / R));
  if (wide)
    hipLaunchKernelGGL((focal_elem_kernel<T, VW, BWD>), grid, dim3(kFocalThreads), 0, s, (const T*)x, ldl, t, d_loss, N, C, gamma, alpha, out, G, R);
  else
    hipLaunchKernelGGL((focal_elem_kernel<T, 1, BWD>), grid, dim3(kFocalThreads), 0, s, (const T*)x, ldl, t, d_loss, N, C, gamma, alpha, out, G, R);
  return hipGetLastError();
}

}  // namespace

// d_loss null: forward (out = loss [N][C]); else backward (out = d_logits [N][C]).  dtype: 0 f32, 1 bf16, 2 half.
hipError_t run_focal_elem(const void* x, int ldl, const long long* t, const float* d_loss, int N, int C, float gamma, float alpha, int dtype,
                          float* out, hipStream_t s) {
  if (dtype == 0) return d_loss ? launch_elem<float, true>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s) : launch_elem<float, false>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s);
  if (dtype == 1) return d_loss ? launch_elem<bf16_t, true>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s) : launch_elem<bf16_t, false>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s);
  if (dtype == 2) return d_loss ? launch_elem<f16_t, true>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s) : launch_elem<f16_t, false>(x, ldl, t, d_loss, N, C, gamma, alpha, out, s);
  return hipErrorInvalidValue;
}

hipError_t run_focal_fused(const float* x, int ldl, const long long* t, const float* w, int N, int C, float gamma, float alpha, float loss_weight,
                           float avg, const int* counts, float* partial, float* out1, float* d, hipStream_t s) {
  int S, rpw, G, R;
  focal_split(N, C, &S, &rpw);
  const bool wide = ldl % 4 == 0 && is16(x) && is16(d);
  focal_map(ldl, wide ? 4 : 1, &G, &R);
  if (wide)
    hipLaunchKernelGGL((focal_fused_kernel<4>), dim3(S), dim3(kFocalThreads), 0, s, x, ldl, t, w, N, C, gamma, alpha, loss_weight, avg, counts, partial, d, G, R, rpw);
  else
    hipLaunchKernelGGL((focal_fused_kernel<1>), dim3(S), dim3(kFocalThreads), 0, s, x, ldl, t, w, N, C, gamma, alpha, loss_weight, avg, counts, partial, d, G, R, rpw);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(focal_merge_kernel, dim3(1), dim3(64), 0, s, partial, S, loss_weight, avg, counts, out1);
  return hipGetLastError();
}

hipError_t run_rpn_focal_loss(const float* o, int ldo, int A, int rows, const long long* labels, const float* label_w, const float* bbox_t,
                              const float* bbox_w, const int* counts, float beta, float gamma, float alpha, float w_cls, float w_bbox, float* out2,
                              float* d_o, hipStream_t s) {
  hipLaunchKernelGGL(rpn_focal_loss_kernel, dim3(1), dim3(1024), 0, s, o, ldo, A, rows, labels, label_w, bbox_t, bbox_w, counts, beta, gamma, alpha,
                     w_cls, w_bbox, out2, d_o);
  return hipGetLastError();
}

}  // namespace hvr
