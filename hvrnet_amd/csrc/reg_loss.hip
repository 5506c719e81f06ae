// Regression and IoU losses for gfx950 (mmdet/models/losses: smooth_l1_loss.py, balanced_l1_loss.py, mse_loss.py, iou_loss.py with
// losses/utils.py weight_reduce_loss; the rules: include/hvr_hip.h "Regression and IoU losses").
// Built with -ffp-contract=off: tests/loss_refs.py bounds every product and sum as a rounding of its own.
//   reg_elem_kernel<RULE>   elementwise family on pred [N][ldp], target / weight / outputs [N][D]: 'none' forward, 'none' backward, or
//                           the reduced form in ONE pass (gradient [N][D] and one f32 partial of sum w l per workgroup).
//   box_pair_kernel<RULE>   box-pair family on pred / target [n][4], one lane per pair, the same three modes.
//   reg_merge_kernel        adds the partials in workgroup order and scales.  No atomics: the result depends on the shape only.
// Row mapping of the elementwise family as in focal.hip: G lanes share a row (its 16-byte pieces, or its elements when a pitch or an
// address rules 16-byte accesses out), 256 / G rows per workgroup step.
#include "common.h"
#include "smooth_l1_dev.h"

namespace hvr {

void focal_split(int N, int C, int* S, int* rows);   // focal.hip: the shape-only split every reduced loss shares

constexpr int kRegThreads = 256;
enum { REG_SMOOTH_L1 = 0, REG_BALANCED_L1 = 1, REG_MSE = 2 };
enum { BOX_IOU = 0, BOX_BOUNDED_IOU = 1 };
enum { MODE_FWD = 0, MODE_BWD = 1, MODE_FUSED = 2 };

struct RegParams { float beta, alpha, gamma, b; };   // SmoothL1: beta.  BalancedL1: all four (b = e^(gamma / alpha) - 1).  MSE: none.
struct BoxParams { float beta, eps; };               // IoU: eps.  BoundedIoU: both.

namespace {

struct LossTerm { float l, g; };

__device__ __forceinline__ float signf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// loss and d loss / d pred of one element at d = pred - target
template <int RULE> __device__ __forceinline__ LossTerm reg_term(float d, const RegParams& p) {
  LossTerm t;
  if constexpr (RULE == REG_SMOOTH_L1) {
    t.l = smooth_l1_term(d, p.beta, 1.f, 1.f, &t.g);
  } else if constexpr (RULE == REG_BALANCED_L1) {
    const float ad = fabsf(d);
    if (ad < p.beta) {
      const float lg = log1pf(p.b * ad / p.beta);
      t.l = p.alpha / p.b * (p.b * ad + 1.f) * lg - p.alpha * ad;
      t.g = (p.alpha * lg + p.alpha * ((1.f - p.beta) / (p.b * ad + p.beta))) * signf(d);   // the second term is exactly 0 at beta = 1
    } else {
      t.l = p.gamma * ad + p.gamma / p.b - p.alpha * p.beta;
      t.g = p.gamma * signf(d);
    }
  } else {
    t.l = d * d;
    t.g = 2.f * d;
  }
  return t;
}

// the smooth-L1 switch of bounded_iou_loss on a term c >= 0: value and slope
__device__ __forceinline__ LossTerm bounded_switch(float c, float beta) {
  LossTerm t;
  t.l = c < beta ? 0.5f * c * c / beta : c - 0.5f * beta;
  t.g = c < beta ? c / beta : 1.f;
  return t;
}

// one axis of bounded_iou_loss: pred (p1, p2), target (t1, t2) -> the centre term and the size term after the switch, and their
// slopes with respect to the pred centre and the pred size
__device__ __forceinline__ void bounded_axis(float p1, float p2, float t1, float t2, const BoxParams& bp, LossTerm* ctr, LossTerm* size) {
  const float pc = (p1 + p2) * 0.5f, tc = (t1 + t2) * 0.5f;
  const float pw = p2 - p1 + 1.f, tw = t2 - t1 + 1.f;
  const float dx = tc - pc, a2 = 2.f * fabsf(dx);
  const float den = tw + a2 + bp.eps;
  const float f = (tw - a2) / den;
  const LossTerm sc = bounded_switch(1.f - fmaxf(f, 0.f), bp.beta);
  ctr->l = sc.l;
  // d(1 - f) / d|dx| = 2 (2 tw + eps) / den^2 where f > 0 (the zero takes the gradient on a tie); d|dx| / d pc = -sign(dx)
  ctr->g = f > 0.f ? sc.g * (2.f * (2.f * tw + bp.eps) / (den * den)) * -signf(dx) : 0.f;
  const float r1 = tw / (pw + bp.eps), r2 = pw / (tw + bp.eps);
  const LossTerm ss = bounded_switch(1.f - fminf(r1, r2), bp.beta);
  size->l = ss.l;
  // the first ratio takes the gradient on a tie
  size->g = r1 <= r2 ? ss.g * (tw / ((pw + bp.eps) * (pw + bp.eps))) : ss.g * (-1.f / (tw + bp.eps));
}

// -log(max(iou, eps)) of one aligned pair and its gradient with respect to the four pred coordinates
__device__ __forceinline__ float iou_term(const float (&p)[4], const float (&t)[4], float eps, float (&g)[4]) {
  const float lx = fmaxf(p[0], t[0]), ly = fmaxf(p[1], t[1]), rx = fminf(p[2], t[2]), ry = fminf(p[3], t[3]);
  const float w = fmaxf(rx - lx + 1.f, 0.f), h = fmaxf(ry - ly + 1.f, 0.f);
  const float I = w * h;
  const float pw = p[2] - p[0] + 1.f, ph = p[3] - p[1] + 1.f;
  const float a1 = pw * ph, a2 = (t[2] - t[0] + 1.f) * (t[3] - t[1] + 1.f);
  const float U = a1 + a2 - I;
  const float iou = I / U;
  g[0] = g[1] = g[2] = g[3] = 0.f;
  if (!(iou >= eps)) return -logf(eps);
  // l = log U - log I: dl = dU / U - dI / I with dU = dA1 - dI.  pred takes the gradient of a max / min on a tie.
  const float dI[4] = {p[0] >= t[0] ? -h : 0.f, p[1] >= t[1] ? -w : 0.f, p[2] <= t[2] ? h : 0.f, p[3] <= t[3] ? w : 0.f};
  const float dA[4] = {-ph, -pw, ph, pw};
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = (dA[k] - dI[k]) / U - dI[k] / I;
  return -logf(iou);
}

__device__ __forceinline__ void load4(const float* p, bool wide, float (&v)[4]) {
  if (wide) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
}
__device__ __forceinline__ void store4(float* p, bool wide, const float (&v)[4]) {
  if (wide) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
  }
}

// the workgroup's sum in the focal order: xor shuffles, then the four waves through LDS in wave order
__device__ __forceinline__ void wg_partial(float acc, float* red, float* partial) {
  const int tid = (int)threadIdx.x;
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

// Workgroup b takes rows [b rpw, min(N, (b + 1) rpw)).  MODE_FWD: out = l.  MODE_BWD: out = dl/dpred * aux (aux = d_loss [N][D]).
// MODE_FUSED: out = (loss_weight / avg * w) dl/dpred, partial[b] = sum w l (aux = w [N][D], nullable).
template <int RULE, int V, int MODE>
__global__ __launch_bounds__(kRegThreads) void reg_elem_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ target,
                                                               const float* __restrict__ aux, int N, int D, RegParams prm, float loss_weight,
                                                               float avg_host, const int* __restrict__ counts, float* __restrict__ partial,
                                                               float* __restrict__ out, int G, int R, int rpw) {
  __shared__ float red[kRegThreads / 64];
  const int tid = (int)threadIdx.x, rib = tid / G, sub = tid - rib * G;
  float scale = 1.f;
  if constexpr (MODE == MODE_FUSED) scale = loss_weight / (counts ? (float)max(counts[0], 1) : avg_host);
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < (long)N ? r0 + rpw : (long)N;
  float acc = 0.f;
  if (rib < R) {
    for (long n = r0 + rib; n < r1; n += R) {
      const float* prow = pred + n * ldp;
      const long o = n * D;
      for (int c0 = sub * V; c0 < D; c0 += G * V) {
        float p[V], t[V], a[V], r[V];
        if constexpr (V == 4) {
          load4(prow + c0, true, p);
          load4(target + o + c0, true, t);
          if (aux) load4(aux + o + c0, true, a);
        } else {
          p[0] = prow[c0]; t[0] = target[o + c0];
          if (aux) a[0] = aux[o + c0];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const LossTerm f = reg_term<RULE>(p[k] - t[k], prm);
          if constexpr (MODE == MODE_FWD) {
            r[k] = f.l;
          } else if constexpr (MODE == MODE_BWD) {
            r[k] = f.g * a[k];
          } else {
            const float w = aux ? a[k] : 1.f;
            acc += w * f.l;
            r[k] = scale * w * f.g;
          }
        }
        if constexpr (V == 4)
          store4(out + o + c0, true, r);
        else
          out[o + c0] = r[0];
      }
    }
  }
  if constexpr (MODE == MODE_FUSED) wg_partial(acc, red, partial);
}

// One lane per pair; workgroup b takes pairs [b rpw, min(n, (b + 1) rpw)).  IoU: loss [n], weight [n].  BoundedIoU: loss and weight
// [n][4].  The gradient is [n][4] in every rule.  MODE as above (aux = d_loss or w, in the loss's shape).
template <int RULE, int MODE>
__global__ __launch_bounds__(kRegThreads) void box_pair_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               const float* __restrict__ aux, int n, BoxParams bp, float loss_weight,
                                                               float avg_host, const int* __restrict__ counts, float* __restrict__ partial,
                                                               float* __restrict__ out, int wide, int rpw) {
  __shared__ float red[kRegThreads / 64];
  float scale = 1.f;
  if constexpr (MODE == MODE_FUSED) scale = loss_weight / (counts ? (float)max(counts[0], 1) : avg_host);
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < (long)n ? r0 + rpw : (long)n;
  float acc = 0.f;
  for (long i = r0 + (long)threadIdx.x; i < r1; i += kRegThreads) {
    float p[4], t[4], l[4], g[4], a[4] = {1.f, 1.f, 1.f, 1.f};
    load4(pred + i * 4, wide & 1, p);
    load4(target + i * 4, wide & 1, t);
    if constexpr (RULE == BOX_IOU) {
      l[0] = iou_term(p, t, bp.eps, g);
      if (aux) a[0] = aux[i];
      if constexpr (MODE == MODE_FWD) {
        out[i] = l[0];
      } else {
        const float c = MODE == MODE_BWD ? a[0] : scale * a[0];
        if constexpr (MODE == MODE_FUSED) acc += a[0] * l[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = c * g[k];
        store4(out + i * 4, wide & 2, g);
      }
    } else {
      LossTerm cx, sx, cy, sy;
      bounded_axis(p[0], p[2], t[0], t[2], bp, &cx, &sx);
      bounded_axis(p[1], p[3], t[1], t[3], bp, &cy, &sy);
      l[0] = cx.l; l[1] = cy.l; l[2] = sx.l; l[3] = sy.l;      // (dx, dy, dw, dh), iou_loss.py:58
      if (aux) load4(aux + i * 4, wide & 4, a);
      if constexpr (MODE == MODE_FWD) {
        store4(out + i * 4, wide & 2, l);
      } else {
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c[k] = MODE == MODE_BWD ? a[k] : scale * a[k];
          if constexpr (MODE == MODE_FUSED) acc += a[k] * l[k];
        }
        // centre = (p1 + p2) / 2, size = p2 - p1 + 1
        const float gcx = 0.5f * (c[0] * cx.g), gcy = 0.5f * (c[1] * cy.g), gsx = c[2] * sx.g, gsy = c[3] * sy.g;
        g[0] = gcx - gsx; g[1] = gcy - gsy; g[2] = gcx + gsx; g[3] = gcy + gsy;
        store4(out + i * 4, wide & 2, g);
      }
    }
  }
  if constexpr (MODE == MODE_FUSED) wg_partial(acc, red, partial);
}

// one wave: lane i adds partials i, i + 64, ... in that order, xor shuffles, out1 = sum * (loss_weight / avg)
__global__ __launch_bounds__(64) void reg_merge_kernel(const float* __restrict__ partial, int S, float loss_weight, float avg_host,
                                                       const int* __restrict__ counts, float* __restrict__ out1) {
  const float avg = counts ? (float)max(counts[0], 1) : avg_host;
  float s = 0.f;
  for (int j = (int)threadIdx.x; j < S; j += 64) s += partial[j];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) out1[0] = s * (loss_weight / avg);
}

namespace {

inline bool is16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int RULE, int MODE>
hipError_t launch_reg(const float* pred, int ldp, const float* target, const float* aux, int N, int D, const RegParams& prm, float loss_weight,
                      float avg, const int* counts, float* partial, float* out, hipStream_t s) {
  int S, rpw;
  focal_split(N, D, &S, &rpw);
  const bool wide = ldp % 4 == 0 && D % 4 == 0 && is16(pred) && is16(target) && is16(out) && (!aux || is16(aux));
  const int V = wide ? 4 : 1;
  int G = (D + V - 1) / V;
  if (G > kRegThreads) G = kRegThreads;
  const int R = kRegThreads / G;
  if (wide)
    hipLaunchKernelGGL((reg_elem_kernel<RULE, 4, MODE>), dim3(S), dim3(kRegThreads), 0, s, pred, ldp, target, aux, N, D, prm, loss_weight, avg, counts,
                       partial, out, G, R, rpw);
  else
    hipLaunchKernelGGL((reg_elem_kernel<RULE, 1, MODE>), dim3(S), dim3(kRegThreads), 0, s, pred, ldp, target, aux, N, D, prm, loss_weight, avg, counts,
                       partial, out, G, R, rpw);
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_reg_rule(int rule, const float* pred, int ldp, const float* target, const float* aux, int N, int D, const RegParams& prm,
                           float loss_weight, float avg, const int* counts, float* partial, float* out, hipStream_t s) {
  if (rule == REG_SMOOTH_L1) return launch_reg<REG_SMOOTH_L1, MODE>(pred, ldp, target, aux, N, D, prm, loss_weight, avg, counts, partial, out, s);
  if (rule == REG_BALANCED_L1) return launch_reg<REG_BALANCED_L1, MODE>(pred, ldp, target, aux, N, D, prm, loss_weight, avg, counts, partial, out, s);
  if (rule == REG_MSE) return launch_reg<REG_MSE, MODE>(pred, ldp, target, aux, N, D, prm, loss_weight, avg, counts, partial, out, s);
  return hipErrorInvalidValue;
}

template <int RULE, int MODE>
hipError_t launch_box(const float* pred, const float* target, const float* aux, int n, const BoxParams& bp, float loss_weight, float avg,
                      const int* counts, float* partial, float* out, hipStream_t s) {
  int S, rpw;
  focal_split(n, 4, &S, &rpw);
  const int wide = (is16(pred) && is16(target) ? 1 : 0) | (is16(out) ? 2 : 0) | (aux && is16(aux) ? 4 : 0);
  hipLaunchKernelGGL((box_pair_kernel<RULE, MODE>), dim3(S), dim3(kRegThreads), 0, s, pred, target, aux, n, bp, loss_weight, avg, counts, partial, out,
                     wide, rpw);
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_box_rule(int rule, const float* pred, const float* target, const float* aux, int n, const BoxParams& bp, float loss_weight,
                           float avg, const int* counts, float* partial, float* out, hipStream_t s) {
  if (rule == BOX_IOU) return launch_box<BOX_IOU, MODE>(pred, target, aux, n, bp, loss_weight, avg, counts, partial, out, s);
  if (rule == BOX_BOUNDED_IOU) return launch_box<BOX_BOUNDED_IOU, MODE>(pred, target, aux, n, bp, loss_weight, avg, counts, partial, out, s);
  return hipErrorInvalidValue;
}

hipError_t launch_merge(const float* partial, int S, float loss_weight, float avg, const int* counts, float* out1, hipStream_t s) {
  hipLaunchKernelGGL(reg_merge_kernel, dim3(1), dim3(64), 0, s, partial, S, loss_weight, avg, counts, out1);
  return hipGetLastError();
}

}  // namespace

// d_loss null: forward (out = loss [N][D]); else backward (out = d_pred [N][D]).  prm4: (beta, alpha, gamma, b).
hipError_t run_reg_elem(int rule, const float* pred, int ldp, const float* target, const float* d_loss, int N, int D, const float* prm4, float* out,
                        hipStream_t s) {
  const RegParams prm{prm4[0], prm4[1], prm4[2], prm4[3]};
  return d_loss ? launch_reg_rule<MODE_BWD>(rule, pred, ldp, target, d_loss, N, D, prm, 1.f, 1.f, nullptr, nullptr, out, s)
                : launch_reg_rule<MODE_FWD>(rule, pred, ldp, target, nullptr, N, D, prm, 1.f, 1.f, nullptr, nullptr, out, s);
}

hipError_t run_reg_fused(int rule, const float* pred, int ldp, const float* target, const float* w, int N, int D, const float* prm4,
                         float loss_weight, float avg, const int* counts, float* partial, float* out1, float* d_pred, hipStream_t s) {
  const RegParams prm{prm4[0], prm4[1], prm4[2], prm4[3]};
  if (hipError_t e = launch_reg_rule<MODE_FUSED>(rule, pred, ldp, target, w, N, D, prm, loss_weight, avg, counts, partial, d_pred, s)) return e;
  int S, rpw;
  focal_split(N, D, &S, &rpw);
  return launch_merge(partial, S, loss_weight, avg, counts, out1, s);
}

// d_loss null: forward (out = loss [n] / [n][4]); else backward (out = d_pred [n][4]).
hipError_t run_box_elem(int rule, const float* pred, const float* target, const float* d_loss, int n, float beta, float eps, float* out,
                        hipStream_t s) {
  const BoxParams bp{beta, eps};
  return d_loss ? launch_box_rule<MODE_BWD>(rule, pred, target, d_loss, n, bp, 1.f, 1.f, nullptr, nullptr, out, s)
                : launch_box_rule<MODE_FWD>(rule, pred, target, nullptr, n, bp, 1.f, 1.f, nullptr, nullptr, out, s);
}

hipError_t run_box_fused(int rule, const float* pred, const float* target, const float* w, int n, float beta, float eps, float loss_weight,
                         float avg, const int* counts, float* partial, float* out1, float* d_pred, hipStream_t s) {
  const BoxParams bp{beta, eps};
  if (hipError_t e = launch_box_rule<MODE_FUSED>(rule, pred, target, w, n, bp, loss_weight, avg, counts, partial, d_pred, s)) return e;
  int S, rpw;
  focal_split(n, 4, &S, &rpw);
  return launch_merge(partial, S, loss_weight, avg, counts, out1, s);
}

}  // namespace hvr
