// Gradient harmonizing losses for gfx950 (mmdet/models/losses/ghm_loss.py GHMC / GHMR; the rules: include/hvr_hip.h "GHM losses").
// Built with -ffp-contract=off: tests/loss_refs.py bounds every product and sum as a rounding of its own.
// Three passes (after a one-wave launch that zeroes the counts) over dense f32 [N][C] matrices taken as E = N C elements, S workgroups of consecutive elements (the shape-only split
// of the reduced losses), nothing read back by the host:
//   ghm_hist_kernel      g per valid element, its bin counted in LDS with integer atomics, ONE integer atomic per bin and workgroup
//                        into counts[bins]; one partial of `tot` per workgroup (GHMC: an integer count, GHMR: the f32 weight sum).
//   ghm_finalize_kernel  one wave: tot (clamped to 1), n = non-empty bins, the momentum update of acc_sum in place, w[bin].
//   ghm_loss_kernel      the same g and bin again, loss term and gradient per element, one f32 partial per workgroup;
//                        ghm_merge_kernel adds the partials in workgroup order: out1 = loss_weight * sum / tot.
// Workspace, in 4-byte words (hvr_ghm_workspace_bytes; include/hvr_hip.h states it for callers):
//   [0, 64) counts int32   [64, 128) w f32   [128] tot f32   [129] n int32   [192, 192 + S) partials (tot, then the loss)
#include "common.h"

namespace hvr {

void focal_split(int N, int C, int* S, int* rows);   // focal.hip

constexpr int kGhmThreads = 256;
constexpr int kGhmMaxBins = 64;
constexpr int kGhmW = 64, kGhmTot = 128, kGhmN = 129, kGhmPartial = 192;

// S workgroups of `per` consecutive elements each (the last may hold fewer, none is empty)
void ghm_split(int N, int C, int* S, long* per) {
  int s, rows;
  focal_split(N, C, &s, &rows);
  const long E = (long)N * C;
  const long p = (E + s - 1) / s;
  *per = p;
  *S = (int)((E + p - 1) / p);
}

namespace {

struct GhmElem { float g, x, t, w, r; bool valid; };   // x: logit (C) or diff (R); r: sqrt(d^2 + mu^2) (R) or sigmoid(x) (C)

// REG false: GHMC (pred = logits; target f32 [N][C], or labels int64 [N] where label k >= 1 marks column k - 1).  REG true: GHMR.
// weight: [N][C], or [N] when w_per_row.
template <bool REG>
__device__ __forceinline__ GhmElem ghm_elem(long e, int C, const float* __restrict__ pred, const float* __restrict__ target,
                                            const long long* __restrict__ labels, const float* __restrict__ weight, int w_per_row, float mu) {
  GhmElem o;
  const long n = e / C;
  o.w = weight[w_per_row ? n : e];
  o.valid = o.w > 0.f;
  if constexpr (REG) {
    o.x = pred[e] - target[e];
    o.t = 0.f;
    o.r = sqrtf(o.x * o.x + mu * mu);
    o.g = fabsf(o.x / o.r);
  } else {
    o.x = pred[e];
    o.t = labels ? (labels[n] == (long long)(e - n * C) + 1 ? 1.f : 0.f) : target[e];
    const float ex = expf(-fabsf(o.x));                 // focal's stable forms: p = 1 / (1 + e) or e / (1 + e)
    const float r = 1.f / (1.f + ex);
    o.r = o.x >= 0.f ? r : ex * r;
    o.g = fabsf(o.r - o.t);
  }
  return o;
}

// bin i iff edges[i] <= g < edges[i + 1]; -1 outside every bin
__device__ __forceinline__ int ghm_bin(float g, const float* edges, int bins) {
  if (!(g >= edges[0]) || !(g < edges[bins])) return -1;
  int lo = 0, hi = bins;                                 // edges[lo] <= g < edges[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (g >= edges[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace

__global__ __launch_bounds__(kGhmMaxBins) void ghm_zero_kernel(int* __restrict__ ws) { ws[threadIdx.x] = 0; }

template <bool REG>
__global__ __launch_bounds__(kGhmThreads) void ghm_hist_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               const long long* __restrict__ labels, const float* __restrict__ weight,
                                                               int w_per_row, long E, int C, float mu, const float* __restrict__ edges, int bins,
                                                               long per, int* __restrict__ ws) {
  __shared__ int cnt[kGhmMaxBins];
  __shared__ float edg[kGhmMaxBins + 1];
  __shared__ float red[kGhmThreads / 64];
  __shared__ int redi[kGhmThreads / 64];
  const int tid = (int)threadIdx.x;
  if (tid < kGhmMaxBins) cnt[tid] = 0;
  if (tid <= bins) edg[tid] = edges[tid];
  __syncthreads();
  const long e0 = (long)blockIdx.x * per;
  const long e1 = e0 + per < E ? e0 + per : E;
  float facc = 0.f;
  int iacc = 0;
  for (long e = e0 + tid; e < e1; e += kGhmThreads) {
    const GhmElem el = ghm_elem<REG>(e, C, pred, target, labels, weight, w_per_row, mu);
    if (REG) facc += el.w;
    if (el.valid) {
      iacc += 1;
      const int b = ghm_bin(el.g, edg, bins);
      if (b >= 0) atomicAdd(&cnt[b], 1);
    }
  }
  if (REG) {
    for (int off = 32; off > 0; off >>= 1) facc += __shfl_xor(facc, off);
    if ((tid & 63) == 0) red[tid >> 6] = facc;
  } else {
    for (int off = 32; off > 0; off >>= 1) iacc += __shfl_xor(iacc, off);
    if ((tid & 63) == 0) redi[tid >> 6] = iacc;
  }
  __syncthreads();
  if (tid < bins && cnt[tid]) atomicAdd(&ws[tid], cnt[tid]);
  if (tid == 0) {
    if (REG)
      reinterpret_cast<float*>(ws)[kGhmPartial + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    else
      ws[kGhmPartial + blockIdx.x] = redi[0] + redi[1] + redi[2] + redi[3];
  }
}

// one wave.  tot: the S partials, lane i takes i, i + 64, ... in that order, xor shuffles; clamped to at least 1.
template <bool REG>
__global__ __launch_bounds__(64) void ghm_finalize_kernel(int* __restrict__ ws, int S, int bins, float momentum, float* __restrict__ acc) {
  const int lane = (int)threadIdx.x;
  float* wsf = reinterpret_cast<float*>(ws);
  float tot;
  if (REG) {
    float s = 0.f;
    for (int j = lane; j < S; j += 64) s += wsf[kGhmPartial + j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    tot = fmaxf(s, 1.f);
  } else {
    int s = 0;                                           // E < 2^31
    for (int j = lane; j < S; j += 64) s += ws[kGhmPartial + j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    tot = fmaxf((float)s, 1.f);
  }
  const int c = lane < bins ? ws[lane] : 0;
  const int n = __popcll(__ballot(c > 0));
  float w = 0.f;
  if (c > 0) {
    float denom = (float)c;
    if (momentum > 0.f) {
      denom = momentum * acc[lane] + (1.f - momentum) * (float)c;
      acc[lane] = denom;
    }
    w = tot / denom / (float)n;
  }
  if (lane < kGhmMaxBins) wsf[kGhmW + lane] = w;
  if (lane == 0) { wsf[kGhmTot] = tot; ws[kGhmN] = n; }
}

template <bool REG>
__global__ __launch_bounds__(kGhmThreads) void ghm_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               const long long* __restrict__ labels, const float* __restrict__ weight,
                                                               int w_per_row, long E, int C, float mu, const float* __restrict__ edges, int bins,
                                                               long per, float loss_weight, const int* __restrict__ ws,
                                                               float* __restrict__ partial, float* __restrict__ d) {
  __shared__ float wbin[kGhmMaxBins];
  __shared__ float edg[kGhmMaxBins + 1];
  __shared__ float red[kGhmThreads / 64];
  const int tid = (int)threadIdx.x;
  const float* wsf = reinterpret_cast<const float*>(ws);
  if (tid < kGhmMaxBins) wbin[tid] = wsf[kGhmW + tid];
  if (tid <= bins) edg[tid] = edges[tid];
  __syncthreads();
  const float tot = wsf[kGhmTot];
  const long e0 = (long)blockIdx.x * per;
  const long e1 = e0 + per < E ? e0 + per : E;
  float acc = 0.f;
  for (long e = e0 + tid; e < e1; e += kGhmThreads) {
    const GhmElem el = ghm_elem<REG>(e, C, pred, target, labels, weight, w_per_row, mu);
    float gr = 0.f;
    if (el.valid) {
      const int b = ghm_bin(el.g, edg, bins);
      if (b >= 0) {
        const float wb = wbin[b];
        if (REG) {
          acc += wb * (el.r - mu);
          gr = loss_weight * wb * (el.x / el.r) / tot;
        } else {
          const float bce = fmaxf(el.x, 0.f) - el.x * el.t + log1pf(expf(-fabsf(el.x)));
          acc += wb * bce;
          gr = loss_weight * wb * (el.r - el.t) / tot;
        }
      }
    }
    d[e] = gr;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void ghm_merge_kernel(const int* __restrict__ ws, const float* __restrict__ partial, int S, float loss_weight,
                                                       float* __restrict__ out1) {
  float s = 0.f;
  for (int j = (int)threadIdx.x; j < S; j += 64) s += partial[j];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) out1[0] = loss_weight * s / reinterpret_cast<const float*>(ws)[kGhmTot];
}

namespace {

template <bool REG>
hipError_t run_ghm(const float* pred, const float* target, const long long* labels, const float* weight, int w_per_row, int N, int C, float mu,
                   const float* edges, int bins, float momentum, float* acc, float loss_weight, int* ws, float* out1, float* d, hipStream_t s) {
  int S;
  long per;
  ghm_split(N, C, &S, &per);
  const long E = (long)N * C;
  // counts are zeroed by a launch of their own, not by a memset: a captured memset node did not zero them on a graph's second replay
  hipLaunchKernelGGL(ghm_zero_kernel, dim3(1), dim3(kGhmMaxBins), 0, s, ws);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL((ghm_hist_kernel<REG>), dim3(S), dim3(kGhmThreads), 0, s, pred, target, labels, weight, w_per_row, E, C, mu, edges, bins, per, ws);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL((ghm_finalize_kernel<REG>), dim3(1), dim3(64), 0, s, ws, S, bins, momentum, acc);
  if (hipError_t e = hipGetLastError()) return e;
  float* partial = reinterpret_cast<float*>(ws) + kGhmPartial;
  hipLaunchKernelGGL((ghm_loss_kernel<REG>), dim3(S), dim3(kGhmThreads), 0, s, pred, target, labels, weight, w_per_row, E, C, mu, edges, bins, per,
                     loss_weight, ws, partial, d);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(ghm_merge_kernel, dim3(1), dim3(64), 0, s, ws, partial, S, loss_weight, out1);
  return hipGetLastError();
}

}  // namespace

size_t ghm_workspace_words(int N, int C) {
  int S;
  long per;
  ghm_split(N, C, &S, &per);
  return (size_t)kGhmPartial + (size_t)S;
}

hipError_t run_ghmc(const float* logits, const float* target, const long long* labels, const float* weight, int w_per_row, int N, int C,
                    const float* edges, int bins, float momentum, float* acc, float loss_weight, void* ws, float* out1, float* d, hipStream_t s) {
  return run_ghm<false>(logits, target, labels, weight, w_per_row, N, C, 0.f, edges, bins, momentum, acc, loss_weight, (int*)ws, out1, d, s);
}

hipError_t run_ghmr(const float* pred, const float* target, const float* weight, int N, int C, float mu, const float* edges, int bins,
                    float momentum, float* acc, float loss_weight, void* ws, float* out1, float* d, hipStream_t s) {
  return run_ghm<true>(pred, target, nullptr, weight, 0, N, C, mu, edges, bins, momentum, acc, loss_weight, (int*)ws, out1, d, s);
}

}  // namespace hvr
