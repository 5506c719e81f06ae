// Soft-NMS read-out on the device: mmdet/ops/nms/src/soft_nms_cpu.pyx (linear / gaussian) as nms_wrapper.py:64-102 calls it, and
// multiclass_nms around it (mmdet/core/post_processing/bbox_nms.py:32-61 with nms_cfg type='soft_nms'), with no host round trip
// (the reference goes .cpu().numpy() per class, nms_wrapper.py:77-79).
//
//   soft_nms_class_kernel  grid (foreground classes, problems), ONE WAVE per workgroup.  The class's candidates (score > score_thr,
//                          ascending row) are compacted into LDS in the reference's physical order, then its rounds run:
//                            round i:  winner = arg max of the scores at positions i .. N-1 (lowest position on equal scores),
//                                      entries i and winner change places, every later entry that overlaps the winner is
//                                      rescored, and the ones that fall below min_score leave the list.
//                          The .pyx removes an entry by moving entry N-1 into its place and looking at that place again; over a
//                          whole round that is a two-pointer compaction: with N' = N - #dead, the dead positions < N' in ascending
//                          order receive the live entries at positions >= N' in DESCENDING order.  So a round is one wave
//                          reduction, one element-wise pass (<= 8 entries per lane) and one ballot compaction; only the rounds are
//                          serial (as many as survivors).
//                          Why one wave: a round has work for at most R - i - 1 <= 511 lanes and is a chain of dependent steps
//                          (reduce -> exchange -> pass -> compaction); a wider workgroup would pay a real workgroup barrier at each of
//                          them, a single wave's barriers are free.  Measured (tools/softnms_bench.py, profiles/softnms_readout.txt):
//                          at most 2.1 us per round with 300 candidates (the launch pair's time, merge included, over the longest
//                          class's rounds; linear; gaussian 2.7 with its f64 exp), class kernel + merge
//                          496 us on the benchmark clip's near-uniform scores (235 rounds in the longest class) against 122 us for
//                          the greedy pair.  A variant of this loop with a 32-bit score reduction + slot ballots in place of the
//                          64-bit (score, position) reduction and 16-byte box reads was SLOWER in the same comparison (533 us) and
//                          was dropped.  A wider workgroup has NOT been measured: one wave is chosen by the argument above, not by a number.
//   soft_nms_merge_kernel  one workgroup per problem: class-major concatenation in selection order with the RESCORED scores, cut to
//                          max_num by (score descending, list position ascending) with the select / sort code of the greedy merge
//                          (nms_dev.h: mc_cut_to_max_num), rows behind *n_out zeroed -- the contract of mc_nms_merge_kernel.
//
// Arithmetic = the compiled .pyx, which mixes f32 and f64: its `cdef float` expressions contain the literal 1, a C double.  So
// x2 - x1 is an f32 subtraction, + 1 and the area products are f64, iw / ih / ua are rounded to f32 once, iw * ih and the quotient
// are f32, the gaussian weight is exp in f64 of an f32 argument, rounded to f32.  This file is built with -ffp-contract=off.
// Plain C++: ballots, shuffles and vector stores only.
#include <atomic>
#include "common.h"
#include "nms_dev.h"

namespace hvr {

constexpr int SN_MAX_R = 512;   // (MC_MAX_R of nms.hip)
constexpr int SN_SLOTS = SN_MAX_R / 64;
enum { SF_X1 = 0, SF_Y1, SF_X2, SF_Y2, SF_SCORE, SF_ROW, SF_N };

__device__ __forceinline__ float sn_max(float a, float b) { return a >= b ? a : b; }   // soft_nms_cpu.pyx:15-19
__device__ __forceinline__ float sn_min(float a, float b) { return a <= b ? a : b; }

// Score of entry (x1, y1, x2, y2, s) after the winner t was taken (soft_nms_cpu.pyx:84-113); *overlaps = whether the entry was
// rescored at all (only then is it tested against min_score).
__device__ __forceinline__ float sn_rescore(float tx1, float ty1, float tx2, float ty2, float x1, float y1, float x2, float y2, float s,
                                            float iou_thr, int method, float sigma, bool* overlaps) {
  *overlaps = false;
  const float iw = (float)((double)(sn_min(tx2, x2) - sn_max(tx1, x1)) + 1.0);
  if (!(iw > 0.f)) return s;
  const float ih = (float)((double)(sn_min(ty2, y2) - sn_max(ty1, y1)) + 1.0);
  if (!(ih > 0.f)) return s;
  const float area = (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));
  const float inter = iw * ih;
  const double tarea = ((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0);
  const float ua = (float)(tarea + (double)area - (double)inter);
  const float ov = inter / ua;
  float weight;
  if (method == 1) {
    weight = ov > iou_thr ? 1.f - ov : 1.f;            // (f32)(1.0 - (f64) ov) is the f32 subtraction
  } else {
    const float arg = (-(ov * ov)) / sigma;
    weight = (float)exp((double)arg);
  }
  *overlaps = true;
  return weight * s;
}

// boxes: row r of problem p at boxes + p * box_pstride + r * box_stride (4 floats); its score at scores + p * score_pstride +
// r * score_stride + class.  out_dets != null is the single-list form (grid 1 x 1): (box, rescored score) rows, int64 input indices
// and the count go straight to the caller's buffers.
__global__ __launch_bounds__(64) void soft_nms_class_kernel(const float* __restrict__ boxes, int box_stride, long box_pstride,
                                                            const float* __restrict__ scores, int score_stride, long score_pstride,
                                                            int R, int use_thr, float score_thr, float iou_thr, int method, float sigma,
                                                            float min_score, float* __restrict__ sel_scores, int* __restrict__ sel_rows,
                                                            int* __restrict__ counts, float* __restrict__ out_dets,
                                                            long long* __restrict__ out_inds, int* __restrict__ n_out) {
  __shared__ uint32_t fld[SF_N][SN_MAX_R];
  __shared__ int hole[SN_MAX_R / 2], srcp[SN_MAX_R / 2];
  const int c = blockIdx.x, p = blockIdx.y, nfg = gridDim.x, lane = threadIdx.x;
  const float* bx = boxes + (long)p * box_pstride;
  const float* sc = scores + (long)p * score_pstride + c;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int N = 0;
  for (int r0 = 0; r0 < R; r0 += 64) {
    const int r = r0 + lane;
    const float s = r < R ? sc[(long)r * score_stride] : 0.f;
    const bool k = r < R && (!use_thr || s > score_thr);
    const unsigned long long m = __ballot(k);
    if (k) {
      const int q = N + (int)__popcll(m & lt);
      const float* b = bx + (long)r * box_stride;
      fld[SF_X1][q] = __float_as_uint(b[0]);
      fld[SF_Y1][q] = __float_as_uint(b[1]);
      fld[SF_X2][q] = __float_as_uint(b[2]);
      fld[SF_Y2][q] = __float_as_uint(b[3]);
      fld[SF_SCORE][q] = __float_as_uint(s);
      fld[SF_ROW][q] = (uint32_t)r;
    }
    N += (int)__popcll(m);
  }
  if (N == 0 && !out_dets) {   // a class without candidates leaves at once
    if (lane == 0) counts[p * nfg + c] = 0;
    return;
  }
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    // ---- winner: highest score at positions [i, N), lowest position on equal scores (`maxscore < s`, strict: -0 == +0) ----
    unsigned long long best = 0ull;
#pragma unroll
    for (int k = 0; k < SN_SLOTS; ++k) {
      const int q = k * 64 + lane;
      if (k * 64 < N && k * 64 + 64 > i && q >= i && q < N) {
        float s = __uint_as_float(fld[SF_SCORE][q]);
        s = s == 0.f ? 0.f : s;
        const unsigned long long key = ((unsigned long long)float_key(s) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)q);
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, o), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
      const unsigned long long other = ((unsigned long long)ohi << 32) | olo;
      best = other > best ? other : best;
    }
    const int winner = __builtin_amdgcn_readfirstlane((int)(0xffffffffu - (uint32_t)best));
    __syncthreads();   // (one wave: orders the reads above against the exchange)
    if (winner != i && lane < SF_N) {
      const uint32_t a = fld[lane][i], b = fld[lane][winner];
      fld[lane][i] = b;
      fld[lane][winner] = a;
    }
    __syncthreads();
    const float tx1 = __uint_as_float(fld[SF_X1][i]), ty1 = __uint_as_float(fld[SF_Y1][i]);
    const float tx2 = __uint_as_float(fld[SF_X2][i]), ty2 = __uint_as_float(fld[SF_Y2][i]);
    // ---- rescore the entries behind i ----
    unsigned long long dm[SN_SLOTS];
    int D = 0;
#pragma unroll
    for (int k = 0; k < SN_SLOTS; ++k) {
      dm[k] = 0ull;
      if (k * 64 < N && k * 64 + 64 > i + 1) {   // wave-uniform
        const int q = k * 64 + lane;
        bool dead = false;
        if (q > i && q < N) {
          bool ovl;
          const float s2 = sn_rescore(tx1, ty1, tx2, ty2, __uint_as_float(fld[SF_X1][q]), __uint_as_float(fld[SF_Y1][q]),
                                      __uint_as_float(fld[SF_X2][q]), __uint_as_float(fld[SF_Y2][q]),
                                      __uint_as_float(fld[SF_SCORE][q]), iou_thr, method, sigma, &ovl);
          if (ovl) {
            fld[SF_SCORE][q] = __float_as_uint(s2);
            dead = s2 < min_score;
          }
        }
        dm[k] = __ballot(dead);
        D += (int)__popcll(dm[k]);
      }
    }
    if (D == 0) continue;   // wave-uniform; every lane re-reads only what it wrote itself
    // ---- compaction: dead positions < N' (ascending) <- live positions >= N' (descending) ----
    const int Nn = N - D;
    int before = 0, tail_dead = 0;
#pragma unroll
    for (int k = 0; k < SN_SLOTS; ++k) {
      if (k * 64 < N && k * 64 + 64 > i + 1) {
        const int q = k * 64 + lane;
        const bool dead = (dm[k] >> lane) & 1ull;
        const int upto = before + (int)__popcll(dm[k] & lt);   // dead entries in front of q
        if (dead && q < Nn) hole[upto] = q;
        if (!dead && q >= Nn && q < N) srcp[(N - 1 - q) - (D - upto)] = q;   // live entries behind q
        const unsigned long long ge = (k * 64 + 64 <= Nn) ? 0ull : (k * 64 >= Nn ? ~0ull : (~0ull << (Nn - k * 64)));
        tail_dead += (int)__popcll(dm[k] & ge);
        before += (int)__popcll(dm[k]);
      }
    }
    const int moves = D - tail_dead;
    __syncthreads();
    for (int j = lane; j < moves; j += 64) {
      const int h = hole[j], s = srcp[j];
      uint32_t v[SF_N];
#pragma unroll
      for (int f = 0; f < SF_N; ++f) v[f] = fld[f][s];
#pragma unroll
      for (int f = 0; f < SF_N; ++f) fld[f][h] = v[f];
    }
    N = Nn;
    __syncthreads();
  }
  __syncthreads();
  if (out_dets) {
    for (int q = lane; q < R; q += 64) {
      const bool in = q < N;
#pragma unroll
      for (int f = 0; f < 5; ++f) out_dets[q * 5 + f] = in ? __uint_as_float(fld[f][q]) : 0.f;
      out_inds[q] = in ? (long long)fld[SF_ROW][q] : 0ll;
    }
    if (lane == 0) *n_out = N;
    return;
  }
  const long base = ((long)p * nfg + c) * R;
  for (int q = lane; q < N; q += 64) {
    sel_scores[base + q] = __uint_as_float(fld[SF_SCORE][q]);
    sel_rows[base + q] = (int)fld[SF_ROW][q];
  }
  if (lane == 0) counts[p * nfg + c] = N;
}

__global__ __launch_bounds__(1024) void soft_nms_merge_kernel(const float* __restrict__ boxes, int R, int nfg,
                                                              const float* __restrict__ sel_scores, const int* __restrict__ sel_rows,
                                                              const int* __restrict__ counts, int max_num, int sp2,
                                                              float* __restrict__ dets, long long* __restrict__ labels,
                                                              int* __restrict__ n_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int offs[128];
  __shared__ int sh_total;
  const int p = blockIdx.x;
  boxes += (long)p * R * 4;
  sel_scores += (long)p * nfg * R;
  sel_rows += (long)p * nfg * R;
  counts += p * nfg;
  dets += (long)p * max_num * 5;
  labels += (long)p * max_num;
  if (threadIdx.x == 0) {
    int t = 0;
    for (int c = 0; c < nfg; ++c) { offs[c] = t; t += counts[c]; }
    sh_total = t;
  }
  __syncthreads();
  const int total = sh_total;
  const int np2 = next_pow2(total > 1 ? total : 1);
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);
  uint32_t* idx = key + np2;  // (class << 16) | place in the class's selection order: ascending == position in the concatenated list
  for (int i = threadIdx.x; i < np2; i += blockDim.x) { key[i] = 0u; idx[i] = 0xffffffffu; }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int c = wave; c < nfg; c += nw) {
    const int pos = offs[c], cnt = counts[c];
    for (int q = lane; q < cnt; q += 64) {
      key[pos + q] = float_key(sel_scores[(long)c * R + q]);
      idx[pos + q] = ((uint32_t)c << 16) | (uint32_t)q;
    }
  }
  __syncthreads();
  const int nout = mc_cut_to_max_num(key, idx, total, np2, max_num, sp2);
  for (int j = threadIdx.x; j < nout; j += blockDim.x) {
    const uint32_t e = idx[j];
    const int c = e >> 16, q = e & 0xffff;
    const int r = sel_rows[(long)c * R + q];
    dets[j * 5 + 0] = boxes[r * 4 + 0];
    dets[j * 5 + 1] = boxes[r * 4 + 1];
    dets[j * 5 + 2] = boxes[r * 4 + 2];
    dets[j * 5 + 3] = boxes[r * 4 + 3];
    dets[j * 5 + 4] = sel_scores[(long)c * R + q];
    labels[j] = c;
  }
  for (int j = nout + threadIdx.x; j < max_num; j += blockDim.x) {
    dets[j * 5 + 0] = dets[j * 5 + 1] = dets[j * 5 + 2] = dets[j * 5 + 3] = dets[j * 5 + 4] = 0.f;
    labels[j] = 0;
  }
  if (threadIdx.x == 0) n_out[p] = nout;
}

// ---------------- launchers ----------------
hipError_t run_soft_nms(const float* dets, int n, float iou_thr, int method, float sigma, float min_score, float* out_dets,
                        long long* inds, int* n_out, hipStream_t s) {
  if (n <= 0 || n > SN_MAX_R) return hipErrorInvalidValue;
  hipLaunchKernelGGL(soft_nms_class_kernel, dim3(1, 1), dim3(64), 0, s, dets, 5, 0L, dets + 4, 5, 0L, n, 0, 0.f, iou_thr, method, sigma,
                     min_score, (float*)nullptr, (int*)nullptr, (int*)nullptr, out_dets, inds, n_out);
  return hipGetLastError();
}

hipError_t run_multiclass_soft_nms(const float* boxes, const float* scores, int P, int R, int ncls, float score_thr, float iou_thr,
                                   int method, float sigma, float min_score, int max_num, float* dets, long long* labels, int* n_out,
                                   const McSoftNmsWs& ws, hipStream_t s) {
  const int nfg = ncls - 1;
  if (R > SN_MAX_R || nfg > 128 || nfg < 1 || R <= 0 || P <= 0 || max_num <= 0) return hipErrorInvalidValue;
  float* sel_scores = ws.sel_scores;
  int *sel_rows = ws.sel_rows, *counts = ws.counts;
  // the merge's LDS, sized for the longest possible list (every candidate of every class survives) as for the greedy merge:
  // survivor list + the select stage's list of next_pow2(max_num) entries; with Soft-NMS a total far above max_num is the NORMAL
  // case, and at R = 300 / 30 classes / max_num = 300 both fit (128 KB + 4 KB), so the cut is a radix select, not a whole-list sort
  const McMergeLds m = mc_merge_lds(nfg * R, max_num);
  if (!m.fits) return hipErrorInvalidValue;
  const int sp2 = m.sp2;
  const size_t lds = m.bytes;
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(soft_nms_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMcMergeLdsCap);
  });
  hipLaunchKernelGGL(soft_nms_class_kernel, dim3(nfg, P), dim3(64), 0, s, boxes, 4, (long)R * 4, scores + 1, ncls, (long)R * ncls, R, 1,
                     score_thr, iou_thr, method, sigma, min_score, sel_scores, sel_rows, counts, (float*)nullptr, (long long*)nullptr,
                     (int*)nullptr);
  hipLaunchKernelGGL(soft_nms_merge_kernel, dim3(P), dim3(1024), lds, s, boxes, R, nfg, sel_scores, sel_rows, counts, max_num, sp2, dets,
                     labels, n_out);
  return hipGetLastError();
}

}  // namespace hvr
