// Device helpers of the NMS kernels shared by nms.hip, tta.hip and softnms.hip: the score sort (descending score, ascending index on ties) and the
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

// The max_num cut of the multiclass read-outs (bbox_nms.py:54-61), shared by the greedy merge (nms.hip) and the Soft-NMS merge
// (softnms.hip): `key` / `idx` hold the concatenated list of `total` entries (key = float_key(score), idx ascending == position in
// the list), padded to np2 with key 0 / idx 0xffffffff, with sp2 * 8 bytes of LDS behind them (sp2 = next_pow2(max_num), or 0 when
// that does not fit: then the whole list is sorted in place).  Returns the number of rows to write; `idx` then points at the list
// to read them from (score descending, list position ascending on equal scores).  Whole workgroup, uniform arguments.
__device__ __forceinline__ int mc_cut_to_max_num(uint32_t* key, uint32_t*& idx, const int total, const int np2, const int max_num,
                                                 const int sp2) {
  int nout = total;
  if (total > max_num && sp2 == 0) {
    // no LDS for the select stage (max_num close to the list length, e.g. the reference's max_num = -1 quirk): sort the
    // whole list in place -- same order (score desc, list position asc), the padding entries (key 0) go last
    bitonic_sort_pairs(key, idx, np2);
    nout = max_num;
  } else if (total > max_num) {
    // top max_num by (score desc, list position asc): radix-select the max_num-th key (4 passes over the LDS list),
    // gather the entries above it plus the first ties, and sort only those (bbox_nms.py:54-61 sorts everything and
    // cuts; the survivors and their order are the same)
    __shared__ int hist[256];
    __shared__ uint32_t sh_prefix, sh_remaining;
    __shared__ int sh_count;
    uint32_t* skey = idx + np2;
    uint32_t* sidx = skey + sp2;
    uint32_t prefix = 0u, remaining = (uint32_t)max_num;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
      __syncthreads();
      const uint32_t himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const uint32_t u = key[i];
        if ((u & himask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t rem = remaining;
        int b = 255;
        for (; b > 0; --b) {
          if ((uint32_t)hist[b] >= rem) break;
          rem -= hist[b];
        }
        sh_prefix = prefix | ((uint32_t)b << shift);
        sh_remaining = rem;
      }
      __syncthreads();
      prefix = sh_prefix;
      remaining = sh_remaining;
      __syncthreads();
    }
    const uint32_t thr_key = prefix;  // key of the max_num-th entry; `remaining` of the entries equal to it are taken
    if (threadIdx.x == 0) sh_count = 0;
    for (int i = threadIdx.x; i < sp2; i += blockDim.x) { skey[i] = 0u; sidx[i] = 0xffffffffu; }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      if (key[i] > thr_key) {
        const int pos = atomicAdd(&sh_count, 1);
        skey[pos] = key[i];
        sidx[pos] = idx[i];
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // ties at the threshold, lowest list position first (the list is in ascending idx order)
      int taken = 0;
      const int base = sh_count;
      for (int i0 = 0; i0 < total && taken < (int)remaining; i0 += 64) {
        const int i = i0 + threadIdx.x;
        const bool eq = i < total && key[i] == thr_key;
        const unsigned long long m = __ballot(eq);
        const int before = __popcll(m & ((1ull << threadIdx.x) - 1ull));
        if (eq && taken + before < (int)remaining) {
          skey[base + taken + before] = thr_key;
          sidx[base + taken + before] = idx[i];
        }
        taken += __popcll(m);
      }
    }
    __syncthreads();
    bitonic_sort_pairs(skey, sidx, sp2);
    idx = sidx;
    nout = max_num;
  }
  return nout;
}

// The merge kernels keep the whole candidate list, next_pow2(candidates) entries of 8 bytes, in LDS, and behind it the select stage's
// list (radix-select the max_num-th score, sort only the entries above it) of next_pow2(max_num) entries.  When that second list does
// not fit beside the first -- max_num close to the list length -- or can never be used (max_num >= every possible survivor count) the
// kernel sorts the survivor list in place instead (sp2 = 0).  One statement for the greedy (nms.hip), Soft-NMS (softnms.hip) and Seq-NMS
// (seqnms.hip) merge launchers and for the entry points' refusal of a list that does not fit (multiclass_nms_max_candidates).
constexpr size_t kMcMergeLdsCap = 160 * 1024 - 3072;
struct McMergeLds { int np2, sp2; size_t bytes; bool fits; };
inline McMergeLds mc_merge_lds(int candidates, int max_num) {
  McMergeLds m;
  for (m.np2 = 1; m.np2 < candidates;) m.np2 <<= 1;
  for (m.sp2 = 1; m.sp2 < max_num;) m.sp2 <<= 1;
  if (max_num >= candidates || (size_t)m.np2 * 8 + (size_t)m.sp2 * 8 > kMcMergeLdsCap) m.sp2 = 0;
  m.bytes = (size_t)m.np2 * 8 + (size_t)m.sp2 * 8;
  m.fits = m.bytes <= kMcMergeLdsCap;
  return m;
}

// ---- workspace layouts of the NMS family (common.h: Carver; a null base is the size query) ----
// run_nms_batched, P problems of n boxes: the score order, the sorted boxes, the mask (whole 64-box chunks: the band form)
struct NmsWs { int* order; float4* boxes4; unsigned long long* mask; size_t bytes; };
inline NmsWs nms_ws(void* base, int P, int n) {
  Carver c(base);
  NmsWs L;
  const size_t nb = (n + 63) / 64;
  L.order = c.take<int>((size_t)P * n);
  L.boxes4 = c.take<float4>((size_t)P * n);
  L.mask = c.take<unsigned long long>((size_t)P * nb * 64 * nb);
  L.bytes = c.off;
  return L;
}

// run_rpn_select_wide, T frames of n_anchor anchors: hist0 and gcount [T][WBINS] each in one buffer (zeroed together), binstart [T][WBINS],
// meta [T][4], done [T] (the band sweep's flags: run_nms_batched's band_done), cand [T][n_anchor]
constexpr int WBINS = 4096;   // score bins
struct RpnWideWs { int *hist0, *gcount, *binstart, *meta, *done; unsigned long long* cand; size_t bytes; };
inline RpnWideWs rpn_wide_ws(void* base, int T, long n_anchor) {
  Carver c(base);
  RpnWideWs L;
  L.hist0 = c.take<int>((size_t)T * WBINS * 2);
  L.gcount = L.hist0 ? L.hist0 + (size_t)T * WBINS : nullptr;
  L.binstart = c.take<int>((size_t)T * WBINS);
  L.meta = c.take<int>((size_t)T * 4);
  L.done = c.take<int>((size_t)T);
  L.cand = c.take<unsigned long long>((size_t)T * n_anchor);
  L.bytes = c.off;
  return L;
}

// run_multiclass_nms: keepflag [ncls - 1][R], kcount [ncls - 1] (the last buffer: counted unrounded, with 256 bytes of slack behind it)
struct McNmsWs { unsigned char* keepflag; int* kcount; size_t bytes; };
inline McNmsWs mc_nms_ws(void* base, int R, int ncls) {
  Carver c(base);
  McNmsWs L;
  L.keepflag = c.take<unsigned char>((size_t)(ncls - 1) * R);
  L.kcount = c.take<int>(0);
  c.skip((size_t)(ncls - 1) * sizeof(int) + 256);
  L.bytes = c.off;
  return L;
}

// run_multiclass_soft_nms, P problems: sel_scores and sel_rows [P][ncls - 1][R], counts [P][ncls - 1]
struct McSoftNmsWs { float* sel_scores; int *sel_rows, *counts; size_t bytes; };
inline McSoftNmsWs mc_soft_nms_ws(void* base, int P, int R, int ncls) {
  Carver c(base);
  McSoftNmsWs L;
  const size_t e = (size_t)P * (ncls - 1) * R;
  L.sel_scores = c.take<float>(e);
  L.sel_rows = c.take<int>(e);
  L.counts = c.take<int>((size_t)P * (ncls - 1));
  c.skip(256);
  L.bytes = c.off;
  return L;
}

// run_seq_nms, F frames in all, W = ceil(R / 64) words per row of boxes: link and ovl [F][R][W]; best, osc and next [ncls - 1][F][R]; alive,
// keep and wmax [ncls - 1][F][W]; with tubes (else null) the per-box (round, length) table [ncls - 1][F][R], the per-(problem, class) round
// counts and their prefix [P][ncls - 1]
struct SeqNmsWs {
  unsigned long long *link, *ovl, *alive, *keep, *wmax;
  float *best, *osc;
  short* next;
  int2* tube;
  int *tcount, *cbase;
  size_t bytes;
};
inline SeqNmsWs seq_nms_ws(void* base, int P, int F, int R, int ncls, bool tubes) {
  Carver c(base);
  SeqNmsWs L;
  const size_t W = (size_t)(R + 63) / 64, g = (size_t)ncls - 1, f = (size_t)F, r = (size_t)R;
  L.link = c.take<unsigned long long>(f * r * W);
  L.ovl = c.take<unsigned long long>(f * r * W);
  L.best = c.take<float>(g * f * r);
  L.osc = c.take<float>(g * f * r);
  L.next = c.take<short>(g * f * r);
  L.alive = c.take<unsigned long long>(g * f * W);
  L.keep = c.take<unsigned long long>(g * f * W);
  L.wmax = c.take<unsigned long long>(g * f * W);
  c.skip(256);   // (slack behind the path kernel's buffers, part of the size since before the tube tables came behind it)
  L.tube = tubes ? c.take<int2>(g * f * r) : nullptr;
  L.tcount = tubes ? c.take<int>((size_t)P * g) : nullptr;
  L.cbase = tubes ? c.take<int>((size_t)P * g) : nullptr;
  L.bytes = c.off;
  return L;
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
