// Seq-NMS read-out of one whole video on the device (Han et al. 2016, "Seq-NMS for Video Object Detection"), as DESIGN.md
// specifies it -- the reference tree has no Seq-NMS, so that specification (restated on the host in tests/seqnms_refs.py) is the
// contract.  Per foreground class: candidates are the rows with score > score_thr; box (t, i) links to box (t + 1, j) iff their
// IoU >= link_thr; repeat { best[t, i] = s[t, i] + max over alive linked j of best[t + 1, j] (backward in time), root = the alive
// box with the largest best (lowest t, then lowest i), the path follows the lowest-j arg max from the root, every path box is
// rescored (sum / length, or the path's largest score), kept and retired together with the alive boxes of its frame that overlap
// it at IoU >= nms_thr } until no candidate is alive.  On a one-frame video that is per-class greedy NMS.
//
//   seq_nms_link_kernel   one wave per (frame, row): row i of frame t gets two bit rows of W = ceil(R / 64) 64-bit words, its links
//                         into frame t + 1 and its overlaps within frame t (ballots of box_iou_plus1 >= thr, the rounded quotient
//                         itself).  The head's boxes are class-agnostic: computed once per video, shared by all classes.
//   seq_nms_path_kernel   one workgroup of W waves per class, thread i = row i.  The dynamic programme is serial in frames (one
//                         workgroup barrier per frame, the next frame's sums double-buffered in LDS) and INCREMENTAL: after a path
//                         that starts in frame r and ends in frame e only frames <= e can change, frames e .. r - 1 are always
//                         recomputed (their own or their successors' alive sets changed) and below r - 1 the sweep stops at the
//                         first frame whose sums all came out unchanged -- from there down neither the alive sets nor the
//                         successor sums differ, so nothing can.  Every wave keeps the maximum of its 64 rows per frame, so the
//                         root is a reduction over F * W values.  The sums are one f32 add per frame and an exact max, whatever
//                         the order: the shortcuts change no bit against the plain loop.  The loop is bounded by the number of
//                         candidates (every round retires its root unconditionally, also a degenerate box whose IoU with itself
//                         is NaN).
//   seq_nms_merge_kernel  one workgroup per frame: class-major list of the kept rows (ascending row) with the RESCORED scores, cut
//                         to max_num with mc_cut_to_max_num, rows behind n_out[t] zeroed -- the contract of mc_nms_merge_kernel.
//
// Problems and tubes.  A call takes P >= 1 independent problems (one video's key frames for one read-out branch):
// problem p owns the frames frame_start[p] .. frame_start[p + 1] - 1 of the stacked inputs.  Every table is indexed by the GLOBAL
// frame, so the link kernel only has to know the last frame of each problem (no links out of it), the path kernel's grid is
// (class, problem) with all pointers moved to the problem's first frame, and the merge is per frame as before.  frame_start is a
// device array of the caller: every kernel clamps what it reads from it to 0 .. Ftot, so a wrong array cannot send a store outside
// the tables.  hvr_seq_nms is the P = 1 case (frame_start = NULL: the one problem is 0 .. Ftot - 1).  With tube outputs the path
// kernel also records, for every path box, the round that selected it (= the tube's index within its class and problem) and, at the
// root, the path length; seq_nms_tube_prefix_kernel turns the per-(problem, class) round counts into id bases; the merge adds the
// base to get the problem-local tube id of every output row and writes one table row per root box.
//
// `phases` of the launcher (1 link, 2 path, 4 merge; hvr_seq_nms runs all three) lets tools/seqnms_bench.py time a kernel alone on
// the workspace the earlier ones filled.  No host read anywhere; the three launches go to the caller's stream with the caller's workspace.  Built with
// -ffp-contract=off (w * h must not fuse into the union).  Plain C++: ballots, shuffles and vector stores only.
#include <atomic>
#include "common.h"
#include "nms_dev.h"

namespace hvr {

constexpr int SQ_MAX_R = 512;   // (MC_MAX_R of nms.hip)
constexpr int SQ_MAX_W = SQ_MAX_R / 64;
constexpr int SQ_MAX_F = 65535;     // frames are the link / merge grids' y / x; (frame, row) packs into 32 bits of the root key
typedef unsigned long long sq_u64;

// the problem of global frame t: the largest p with frame_start[p] <= t (a bounded search, whatever the array holds) and its frame
// range [f0, f1) clamped to 0 .. F.  frame_start == NULL: one problem, all F frames.
__device__ __forceinline__ int sq_problem_of(const int* __restrict__ frame_start, int P, int F, int t, int& f0, int& f1) {
  f0 = 0;
  f1 = F;
  if (!frame_start) return 0;
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frame_start[mid] <= t) lo = mid; else hi = mid - 1;
  }
  f0 = min(max(frame_start[lo], 0), F);
  f1 = min(max(frame_start[lo + 1], f0), F);
  return lo;
}

__global__ __launch_bounds__(256) void seq_nms_link_kernel(const float4* __restrict__ boxes, const int* __restrict__ frame_start, int P,
                                                           int F, int R, int W, float link_thr, float nms_thr,
                                                           sq_u64* __restrict__ link, sq_u64* __restrict__ ovl) {
  const int t = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= R) return;   // wave-uniform
  const float4 a = boxes[(long)t * R + i];
  int f0, f1;
  sq_problem_of(frame_start, P, F, t, f0, f1);
  const bool has_next = t + 1 < f1;   // the last frame of a problem has no links (f1 <= F: the next frame's loads stay inside)
  sq_u64 lw = 0ull, ow = 0ull;   // lane k ends up with word k
  for (int k = 0; k < W; ++k) {
    const int j = k * 64 + lane;
    bool l = false, o = false;
    if (j < R) {
      o = box_iou_plus1(a, boxes[(long)t * R + j]) >= nms_thr;
      if (has_next) l = box_iou_plus1(a, boxes[(long)(t + 1) * R + j]) >= link_thr;
    }
    const sq_u64 lm = __ballot(l), om = __ballot(o);
    if (lane == k) { lw = lm; ow = om; }
  }
  if (lane < W) {
    link[((long)t * R + i) * W + lane] = lw;
    ovl[((long)t * R + i) * W + lane] = ow;
  }
}

__device__ __forceinline__ sq_u64 sq_wave_max(sq_u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    const sq_u64 other = ((sq_u64)ohi << 32) | olo;
    v = other > v ? other : v;
  }
  return v;
}

// grid (class, problem), blockDim.x = 64 * W; scores: s[t, i] of class blockIdx.x at scores[((long)t * R + i) * ncls + 1 + blockIdx.x].
// Below, F and every frame index are the PROBLEM's: all pointers are moved to its first frame f0 of the Ftot stacked ones.
// tube_g (NULL = no tube outputs): per path box (round that selected it, path length at the root / 0 elsewhere); tcount: the
// rounds of this (problem, class).
__global__ __launch_bounds__(SQ_MAX_R) void seq_nms_path_kernel(const float* __restrict__ scores, const int* __restrict__ frame_start,
                                                                int Ftot, int R, int W, int ncls, float score_thr, int rescore_max,
                                                                const sq_u64* __restrict__ link_g, const sq_u64* __restrict__ ovl_g,
                                                                float* __restrict__ best_g, short* __restrict__ next_g,
                                                                float* __restrict__ osc_g, sq_u64* __restrict__ alive_g,
                                                                sq_u64* __restrict__ keep_g, sq_u64* __restrict__ wmax_g,
                                                                int2* __restrict__ tube_g, int* __restrict__ tcount) {
  __shared__ float bestL[2][SQ_MAX_R];
  __shared__ int chg[3];
  __shared__ sq_u64 red[SQ_MAX_W];
  __shared__ int cnt[SQ_MAX_W];
  const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int f0 = 0, f1 = Ftot;
  if (frame_start) {
    f0 = min(max(frame_start[blockIdx.y], 0), Ftot);
    f1 = min(max(frame_start[blockIdx.y + 1], f0), Ftot);
  }
  const int F = f1 - f0;
  const long row0 = ((long)c * Ftot + f0) * R, word0 = ((long)c * Ftot + f0) * W;
  const float* sc = scores + (long)f0 * R * ncls + 1 + c;
  const sq_u64* link = link_g + (long)f0 * R * W;
  const sq_u64* ovl = ovl_g + (long)f0 * R * W;
  float* best = best_g + row0;
  short* next = next_g + row0;
  float* osc = osc_g + row0;
  int2* tube = tube_g ? tube_g + row0 : nullptr;
  sq_u64* alive = alive_g + word0;
  sq_u64* keep = keep_g + word0;
  sq_u64* wmax = wmax_g + word0;

  // ---- candidates ----
  int mine = 0;
  for (int t = 0; t < F; ++t) {
    const float s = tid < R ? sc[((long)t * R + tid) * ncls] : 0.f;
    const sq_u64 m = __ballot(tid < R && s > score_thr);   // (a NaN score is no candidate)
    if (lane == 0) {
      alive[(long)t * W + wave] = m;
      keep[(long)t * W + wave] = 0ull;
    }
    mine += (int)__popcll(m);
  }
  if (lane == 0) cnt[wave] = mine;
  __syncthreads();
  int N = 0;
  for (int w = 0; w < W; ++w) N += cnt[w];

  int e = F - 1, rt = F;
  bool first = true;
  int it = 0;   // the round counter: a tube's index within its class and problem
  for (; it < N; ++it) {   // every round retires its root: at most N rounds
    // ---- sums: frames e .. 0, stopping early below the last path's root frame ----
    if (e + 1 < F && tid < R) bestL[(e + 1) & 1][tid] = best[(long)(e + 1) * R + tid];
    if (tid < 3) chg[tid] = 0;
    __syncthreads();
    int step = 0;
    for (int t = e; t >= 0; --t, ++step) {
      const bool al = (alive[(long)t * W + wave] >> lane) & 1ull;
      sq_u64 key = 0ull;
      bool changed = false;
      if (al) {
        float m = 0.f;
        int nx = -1;
        if (t + 1 < F) {
          const sq_u64* lk = link + ((long)t * R + tid) * W;
          const sq_u64* an = alive + (long)(t + 1) * W;
          const float* bn = bestL[(t + 1) & 1];
          for (int k = 0; k < W; ++k) {
            sq_u64 b = lk[k] & an[k];
            while (b) {   // ascending j: the lowest j wins on equal sums (every sum is > 0)
              const int j = k * 64 + (int)__ffsll(b) - 1;
              b &= b - 1ull;
              const float v = bn[j];
              if (v > m) { m = v; nx = j; }
            }
          }
        }
        const float nb = sc[((long)t * R + tid) * ncls] + m;
        changed = first || __float_as_uint(best[(long)t * R + tid]) != __float_as_uint(nb);
        best[(long)t * R + tid] = nb;
        next[(long)t * R + tid] = (short)nx;
        bestL[t & 1][tid] = nb;
        key = ((sq_u64)float_key(nb) << 32) | (sq_u64)(0xffffffffu - ((uint32_t)t * (uint32_t)SQ_MAX_R + (uint32_t)tid));
      }
      key = sq_wave_max(key);
      if (lane == 0) wmax[(long)t * W + wave] = key;
      if (changed) chg[step % 3] = 1;
      if (tid == 0) chg[(step + 1) % 3] = 0;
      __syncthreads();
      if (!first && t <= rt - 1 && !chg[step % 3]) break;   // uniform
    }
    first = false;
    // ---- root: largest sum, lowest frame, lowest row ----
    sq_u64 k = 0ull;
    for (long q = tid; q < (long)F * W; q += blockDim.x) {
      const sq_u64 v = wmax[q];
      k = v > k ? v : k;
    }
    k = sq_wave_max(k);
    if (lane == 0) red[wave] = k;
    __syncthreads();
    k = 0ull;
    for (int w = 0; w < W; ++w) k = red[w] > k ? red[w] : k;
    if (k == 0ull) break;   // nothing alive (uniform)
    const uint32_t pos = 0xffffffffu - (uint32_t)k;
    rt = (int)(pos / (uint32_t)SQ_MAX_R);
    const int r0 = (int)(pos % (uint32_t)SQ_MAX_R);
    const float root_best = __uint_as_float((uint32_t)(k >> 32) & 0x7fffffffu);   // (sums are positive: float_key set the top bit)
    // ---- path: every thread walks it (uniform loads); threads < W retire word tid of the frame ----
    int n = 0, tt = rt, rr = r0;
    float mx = 0.f;
    while (rr >= 0 && tt < F) {
      ++n;
      if (rescore_max) {
        const float s = sc[((long)tt * R + rr) * ncls];
        mx = s > mx ? s : mx;
      }
      if (tid < W) {
        sq_u64 o = ovl[((long)tt * R + rr) * W + tid];
        const sq_u64 self = tid == (rr >> 6) ? 1ull << (rr & 63) : 0ull;
        alive[(long)tt * W + tid] &= ~(o | self);   // the path box leaves unconditionally (its IoU with itself may be NaN)
        if (self) keep[(long)tt * W + tid] |= self;
      }
      rr = next[(long)tt * R + rr];
      ++tt;
    }
    e = tt - 1;
    const float out = rescore_max ? mx : root_best / (float)n;
    tt = rt;
    rr = r0;
    while (rr >= 0 && tt < F) {
      if (tid == 0) {
        osc[(long)tt * R + rr] = out;
        if (tube) tube[(long)tt * R + rr] = make_int2(it, tt == rt ? n : 0);
      }
      rr = next[(long)tt * R + rr];
      ++tt;
    }
  }
  if (tcount && tid == 0) tcount[(long)blockIdx.y * gridDim.x + c] = it;   // (a round that found nothing alive left the loop before ++it)
}

// per problem the exclusive prefix of the round counts over its classes (cbase: the first tube id of a class), then the exclusive
// prefix of the problems' totals (tube_start [P + 1]; the last entry is the true total).  One workgroup.
__global__ __launch_bounds__(256) void seq_nms_tube_prefix_kernel(const int* __restrict__ tcount, int P, int nfg, int* __restrict__ cbase,
                                                                  int* __restrict__ tube_start) {
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    int s = 0;
    for (int c = 0; c < nfg; ++c) {
      cbase[(long)p * nfg + c] = s;
      s += tcount[(long)p * nfg + c];
    }
    tube_start[p + 1] = s;   // the problem's total, until the scan below replaces it
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int p = 0; p < P; ++p) {
      const int total = tube_start[p + 1];
      tube_start[p] = run;
      run += total;
    }
    tube_start[P] = run;
  }
}

__global__ __launch_bounds__(1024) void seq_nms_merge_kernel(const float* __restrict__ boxes, int F, int R, int W, int nfg,
                                                             const float* __restrict__ osc, const sq_u64* __restrict__ keep,
                                                             int max_num, int sp2, float* __restrict__ dets,
                                                             long long* __restrict__ labels, int* __restrict__ n_out,
                                                             const int* __restrict__ frame_start, int P, const int2* __restrict__ tube_g,
                                                             const int* __restrict__ cbase, const int* __restrict__ tube_start,
                                                             int* __restrict__ tube_ids, int4* __restrict__ tubes,
                                                             float* __restrict__ tube_scores, int max_tubes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int offs[128], cnts[128], cb[128];
  __shared__ int sh_total;
  const int t = blockIdx.x;
  // tube outputs (tube_ids != NULL): this frame's problem p, its first frame f0, its first table row and its classes' id bases
  int p = 0, f0 = 0, f1, row0 = 0;
  if (tube_ids) {
    p = sq_problem_of(frame_start, P, F, t, f0, f1);
    row0 = tube_start[p];
    if ((int)threadIdx.x < nfg) cb[threadIdx.x] = cbase[(long)p * nfg + threadIdx.x];
    tube_ids += (long)t * max_num;
  }
  boxes += (long)t * R * 4;
  dets += (long)t * max_num * 5;
  labels += (long)t * max_num;
  if ((int)threadIdx.x < nfg) {
    int n = 0;
    for (int k = 0; k < W; ++k) n += (int)__popcll(keep[((long)threadIdx.x * F + t) * W + k]);
    cnts[threadIdx.x] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int c = 0; c < nfg; ++c) { offs[c] = s; s += cnts[c]; }
    sh_total = s;
  }
  __syncthreads();
  const int total = sh_total;
  const int np2 = next_pow2(total > 1 ? total : 1);
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);
  uint32_t* idx = key + np2;  // (class << 16) | row: ascending == position in the concatenated list
  for (int i = threadIdx.x; i < np2; i += blockDim.x) { key[i] = 0u; idx[i] = 0xffffffffu; }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int c = wave; c < nfg; c += nw) {
    int pos = offs[c];
    for (int k = 0; k < W; ++k) {
      const sq_u64 m = keep[((long)c * F + t) * W + k];
      if ((m >> lane) & 1ull) {
        const int r = k * 64 + lane;
        const int q = pos + (int)__popcll(m & ((1ull << lane) - 1ull));
        key[q] = float_key(osc[((long)c * F + t) * R + r]);
        idx[q] = ((uint32_t)c << 16) | (uint32_t)r;
        if (tube_ids) {   // a root box writes its tube's table row (every tube has one root: every row is written once)
          const int2 tu = tube_g[((long)c * F + t) * R + r];
          const long row = (long)row0 + cb[c] + tu.x;
          if (tu.y > 0 && row >= 0 && row < (long)max_tubes) {
            tubes[row] = make_int4(p, c, t - f0, tu.y);
            tube_scores[row] = osc[((long)c * F + t) * R + r];
          }
        }
      }
      pos += (int)__popcll(m);
    }
  }
  __syncthreads();
  const int nout = mc_cut_to_max_num(key, idx, total, np2, max_num, sp2);
  for (int j = threadIdx.x; j < nout; j += blockDim.x) {
    const uint32_t en = idx[j];
    const int c = en >> 16, r = en & 0xffff;
    dets[j * 5 + 0] = boxes[r * 4 + 0];
    dets[j * 5 + 1] = boxes[r * 4 + 1];
    dets[j * 5 + 2] = boxes[r * 4 + 2];
    dets[j * 5 + 3] = boxes[r * 4 + 3];
    dets[j * 5 + 4] = osc[((long)c * F + t) * R + r];
    labels[j] = c;
    if (tube_ids) tube_ids[j] = cb[c] + tube_g[((long)c * F + t) * R + r].x;
  }
  for (int j = nout + threadIdx.x; j < max_num; j += blockDim.x) {
    dets[j * 5 + 0] = dets[j * 5 + 1] = dets[j * 5 + 2] = dets[j * 5 + 3] = dets[j * 5 + 4] = 0.f;
    labels[j] = 0;
    if (tube_ids) tube_ids[j] = -1;
  }
  if (threadIdx.x == 0) n_out[t] = nout;
}

// ---------------- launchers ----------------
// P problems of frame_start [P + 1] (device; NULL: one problem of all F frames), F frames in all.  tube_ids != NULL: the four tube
// outputs (all four non-NULL then; ws is then the layout with its tube tables, nms_dev.h: seq_nms_ws).
hipError_t run_seq_nms(const float* boxes, const float* scores, int P, const int* frame_start, int F, int R, int ncls, float score_thr,
                       float link_thr, float nms_thr, int rescore_max, int max_num, float* dets, long long* labels, int* n_out,
                       int* tube_ids, int* tubes, float* tube_scores, int* tube_start, int max_tubes, const SeqNmsWs& ws, int phases, hipStream_t s) {
  const int nfg = ncls - 1;
  if (R > SQ_MAX_R || R <= 0 || nfg > 128 || nfg < 1 || F <= 0 || F > SQ_MAX_F || max_num <= 0 || P < 1 || P > F || (!frame_start && P != 1))
    return hipErrorInvalidValue;
  const int W = (R + 63) / 64;
  sq_u64 *link = ws.link, *ovl = ws.ovl, *alive = ws.alive, *keep = ws.keep, *wmax = ws.wmax;
  float *best = ws.best, *osc = ws.osc;
  short* next = ws.next;
  if ((tube_ids != nullptr) != (ws.tube != nullptr)) return hipErrorInvalidValue;
  int2* tube = ws.tube;
  int *tcount = ws.tcount, *cbase = ws.cbase;
  // the merge's LDS as for the other read-outs: the longest possible list (every candidate of every class kept) + the select list
  const McMergeLds m = mc_merge_lds(nfg * R, max_num);
  if (!m.fits) return hipErrorInvalidValue;
  const int sp2 = m.sp2;
  const size_t lds = m.bytes;
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(seq_nms_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMcMergeLdsCap);
  });
  if (phases & 1) hipLaunchKernelGGL(seq_nms_link_kernel, dim3((R + 3) / 4, F), dim3(256), 0, s, (const float4*)boxes, frame_start, P, F, R, W, link_thr, nms_thr,
                     link, ovl);
  if (phases & 2) hipLaunchKernelGGL(seq_nms_path_kernel, dim3(nfg, P), dim3(64 * W), 0, s, scores, frame_start, F, R, W, ncls, score_thr, rescore_max, link,
                     ovl, best, next, osc, alive, keep, wmax, tube, tcount);
  if ((phases & 4) && tube_ids) hipLaunchKernelGGL(seq_nms_tube_prefix_kernel, dim3(1), dim3(256), 0, s, tcount, P, nfg, cbase, tube_start);
  if (phases & 4) hipLaunchKernelGGL(seq_nms_merge_kernel, dim3(F), dim3(1024), lds, s, boxes, F, R, W, nfg, osc, keep, max_num, sp2, dets, labels, n_out,
                     frame_start, P, tube, cbase, tube_start, tube_ids, (int4*)tubes, tube_scores, max_tubes);
  return hipGetLastError();
}

}  // namespace hvr
